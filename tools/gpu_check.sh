#!/bin/bash
# GPU-box smoke: parity tests, two bench runs, kernel trace.  usage: tools/gpu_check.sh <output dir>
O=${1:?usage: tools/gpu_check.sh <output dir>}
mkdir -p $O
timeout 900 python -m pytest tests -m gpu -x -q > $O/tests.log 2>&1; echo "tests rc=$?"
tail -3 $O/tests.log
for i in a b; do
  timeout 300 python bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $O/bench_$i.log 2>&1
  tail -1 $O/bench_$i.log | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('bench', round(d['value'],2), d['unit'], d['ms_per_step'], d.get('roofline'))"
done
R=$(pwd); A=$(cd $O && pwd); cd /tmp && export TMPDIR=/tmp
timeout 600 rocprofv3 --kernel-trace --stats -d $A/prof -o p -- python $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-profile > $A/prof.log 2>&1
cd $R; python profiles/summarize_rocpd.py $O/prof/p_results.db $O/kernel_stats.csv > /dev/null 2>&1
python - <<PY
import csv
for r in list(csv.DictReader(open("$O/kernel_stats.csv")))[:11]:
    print(f"{float(r['avg_us']):9.2f} us x{r['calls']:>5}  {r['percent']:>6}%  {r['kernel'][:90]}")
PY
python tools/parity_report.py > $O/parity.md 2>&1; tail -12 $O/parity.md

#!/usr/bin/env python
"""Distribution metrics on one GPU: ``cmmd`` and ``FeatureBank.moments`` at 5 000 and 30 000 rows of width 768.

    python tools/metrics_bench.py [--rows 5000 30000] [--dim 768] [--iters 5] [--out profiles/metrics_bench.txt]

Times are HIP events around whole calls.  ``cmmd`` is three pair sums (two same-set, one cross); the pair kernel's rate is reported by
2 na nb dim over ALL pairs of the three sums, although a same-set sum runs only the tiles on or above the diagonal -- so the figure is the useful
rate, not the MFMA rate (that one is ``mfma_tflops``, by the tiles that ran).  The comparison point is the float64 statement through ``torch.cdist`` on
the same device, in row chunks of 5 000 (the parent commit has no path of its own): ``expm1(-gamma cdist(x, y)^2).sum()`` three times."""
import argparse, json, os, sys
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformer_latent_diffusion_amd import FeatureBank, _lib, cmmd          # noqa: E402
from transformer_latent_diffusion_amd.metrics import kernel_sum             # noqa: E402

PEAK_F32_MATRIX = 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, nargs="+", default=[5000, 30000])
ap.add_argument("--dim", type=int, default=768)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def timed(fn, iters):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


def cdist_sum(x, y, gamma, chunk=5000):
    total = torch.zeros((), dtype=torch.float64, device=x.device)
    for i in range(0, len(x), chunk):
        total += torch.expm1(-gamma * torch.cdist(x[i:i + chunk], y) ** 2).sum()
    return total


def cdist_mmd2(x, y, gamma):
    n, m = len(x), len(y)
    return cdist_sum(x, x, gamma) / (n * n) + cdist_sum(y, y, gamma) / (m * m) - 2.0 * cdist_sum(x, y, gamma) / (n * m)


lines = []
g = torch.Generator(device="cuda").manual_seed(0)
for n in a.rows:
    banks = []
    for shift in (0.0, 0.05):
        b = FeatureBank(a.dim, n, "cuda")
        b.add(torch.randn(n, a.dim, device="cuda", generator=g) + shift)
        banks.append(b)
    x, y = banks
    dt_append = timed(lambda: FeatureBank(a.dim, n, "cuda").add(x.features().contiguous()), a.iters)
    dt_cmmd = timed(lambda: cmmd(x, y), a.iters)
    dt_cross = timed(lambda: kernel_sum(x, y, 0.005), a.iters)
    dt_same = timed(lambda: kernel_sum(x, x, 0.005), a.iters)
    dt_mom = timed(lambda: x.moments(), a.iters)
    value = float(cmmd(x, y))
    x64, y64 = x.features().double(), y.features().double()
    dt_ref = timed(lambda: cdist_mmd2(x64, y64, 0.005), 1)
    ref = 1000.0 * float(cdist_mmd2(x64, y64, 0.005))
    L = _lib.lib()
    tiles = 2 * L.tld_feat_kernel_sum_partials(n, n, 1) + L.tld_feat_kernel_sum_partials(n, n, 0)
    pitch = x.pitch
    lines.append({"metric": "cmmd_ms", "value": dt_cmmd * 1e3, "unit": "ms", "rows": n, "dim": a.dim,
                  "pair_tflops_by_2_na_nb_dim": 3 * 2.0 * n * n * a.dim / dt_cmmd / 1e12, "mfma_tflops": tiles * 2.0 * 128 * 128 * pitch / dt_cmmd / 1e12,
                  "mfma_fraction_of_f32_matrix_peak": tiles * 2.0 * 128 * 128 * pitch / dt_cmmd / PEAK_F32_MATRIX,
                  "cross_sum_ms": dt_cross * 1e3, "cross_sum_tflops": 2.0 * n * n * a.dim / dt_cross / 1e12, "same_sum_ms": dt_same * 1e3,
                  "moments_ms": dt_mom * 1e3, "moments_gflops": 2.0 * n * a.dim * a.dim / dt_mom / 1e9, "append_ms": dt_append * 1e3,
                  "cdist_float64_ms": dt_ref * 1e3, "speedup_over_cdist_float64": dt_ref / dt_cmmd, "cmmd": value, "cmmd_cdist_float64": ref,
                  "cmmd_difference": abs(value - ref), "data": "synthetic (unit rows of randn, the second set shifted by 0.05)"})
    print(json.dumps(lines[-1]), flush=True)
    del x64, y64
if a.out:
    with open(a.out, "w") as f:
        f.write("tools/metrics_bench.py: cmmd (three pair sums on the fp32 MFMA) and bank moments, HIP-event times; comparison: float64 torch.cdist on the same device\n")
        for ln in lines:
            f.write(json.dumps(ln) + "\n")

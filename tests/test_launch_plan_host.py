"""CPU: the launches of the inference forward's row and attention kernels -- csrc/tld_launch_plan.h through
tests/host/launch_plan_main.cpp, built by the host compiler plain and under AddressSanitizer + UBSan, against the restatement in tests/launch_plan_ref.py
field by field over a dense sweep; that no LDS figure passes a CU's 160 KiB at a configuration tld_engine_create accepts; that no grid extent passes the
launch's limits wherever create and the two raw-buffer hooks accept; that the launch-path bits of the plans, combined as run_body combines the launches
under a BodyPlan (tests/host/body_plan_main.cpp), are the bits tests/test_forward_grids_host.py expects of every case of its tables; and that no plan of
the body-plan sweep that asks for the quantising LayerNorm, cross_row's extra outputs or the split-K finish meets a width without that kernel."""
import itertools
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import pytest

import body_plan_ref as BP
import launch_plan_ref as LP
import test_body_plan_host as TB
import test_forward_grids_host as HG
import test_gpu_forward_stages as FS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DS = list(range(64, 1025, 64))
GRIDS = list(range(4, 65, 4))
NTOKS = sorted({32, 64, 128} | {G * G for G in GRIDS})              # 32, 64, 128 and every 16 k^2 up to 4096
BATCHES = list(range(1, 9)) + [15, 29, 64, 128]
CUS = (256, 304)
PDS = (4, 16, 48, 64)
PATCH = {4: (4, 1), 16: (4, 2), 48: (12, 2), 64: (16, 2)}           # pd -> (n_channels, patch_size)
BOOLS = (0, 1)


def _build(tmp, name):
    """tests/host/<name>.cpp built twice (run directly, nothing preloaded); ``run(lines)`` returns the output lines, the same from both builds."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    src = [os.path.join(REPO, "tests", "host", name + ".cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"{name}_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exes[tag]], check=True)

    def run(lines):
        path = tmp / f"{name}_cases_{len(os.listdir(tmp))}.txt"
        path.write_text("".join(ln + "\n" for ln in lines))
        outs = []
        for tag, exe in exes.items():
            r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
            outs.append(r.stdout)
        assert outs[0] == outs[1], "the sanitizer build answers differently"
        res = outs[0].splitlines()
        assert len(res) == len(lines)
        return res

    return run


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("launch_plan"), "launch_plan_main")


@pytest.fixture(scope="module")
def body_driver(tmp_path_factory):
    run = _build(tmp_path_factory.mktemp("launch_body_plan"), "body_plan_main")
    return lambda lines: [json.loads(ln) for ln in run(lines)]


def _plans(driver, cases):
    """[(site, args)] -> the header's plans as dicts (the two hooks' "refused" flag under that key)."""
    out = []
    for (site, args), ln in zip(cases, driver([" ".join(map(str, (site, *args))) for site, args in cases])):
        v = [int(t) for t in ln.split()]
        names = LP.FIELDS[site] + (("refused",) if site in ("dw", "attn") else ())
        assert len(v) == len(names), (site, args, ln)
        out.append(dict(zip(names, v)))
    return out


def _sweep():
    for d, n, b, pd, held in itertools.product(DS, NTOKS, BATCHES, PDS, BOOLS):
        yield "embed", (b, n, pd, pd, d, held)
    for d, held in itertools.product(DS, BOOLS):                    # (a conv patch that is not the Linear's input width: the plain kernel)
        yield "embed", (3, 256, 16, 4, d, held)
    for d, n, b, mx8 in itertools.product(DS, NTOKS, BATCHES, BOOLS):
        yield "ln", (b * n, d, mx8)
    for d, n, b, cus, x_in, f8 in itertools.product(DS, NTOKS + [8, 24, 40], BATCHES, CUS, BOOLS, BOOLS):      # (8, 24, 40: no multiple of 16)
        yield "cross", (b, n, d, d // 64, x_in, f8, cus)
    for d, n, b in itertools.product(DS, NTOKS, BATCHES):
        yield "skf", (b * n, d)
    for d, n, b, pd, hid, held, cus in itertools.product(DS, NTOKS, BATCHES, PDS, BOOLS, BOOLS, CUS):
        yield "tail", (b, n, pd, d, hid, held, cus)
    for b, G, ch, f8 in itertools.product(BATCHES, GRIDS + [96], (64, 128, 1024), BOOLS):
        yield "dw", (b, G, ch, f8)
    for b, n, H in itertools.product(BATCHES, NTOKS, (1, 2, 3, 4, 12, 16)):
        yield "attn", (b, n, H)


@pytest.fixture(scope="module")
def swept(driver):
    cases = list(_sweep())
    return cases, _plans(driver, cases)


def test_sweep_against_the_restatement(swept):
    cases, got = swept
    seen = set()
    for (site, args), g in zip(cases, got):
        g = {k: v for k, v in g.items() if k != "refused"}
        assert g == LP.PLANS[site](*args), (site, args)
        seen.add((site, g["form"]))
    # every form of every site, the "no such kernel" ones included
    assert seen == {(s, f) for s, n in (("embed", 2), ("ln", 4), ("cross", 2), ("skf", 3), ("tail", 3), ("dw", 3), ("attn", 4)) for f in range(n)}
    by = {(site, args): g for (site, args), g in zip(cases, got)}
    # by name: the shapes of the benchmark (d 768, 16 x 16 tokens, batch 128, 256 CUs) and the partitions the grid tests run
    c1 = by["cross", (128, 256, 768, 12, 0, 0, 256)]
    assert (c1["form"], c1["nq"], c1["gpw"], c1["gx"], c1["block"], c1["lds"]) == (1, 3, 8, 256, 512, 2 * 16 * 768 * 2 + 8192 + 2 * 768 * 4)
    t1 = by["tail", (128, 256, 16, 768, 1, 1, 256)]
    assert (t1["form"], t1["nt"], t1["rt"], t1["gx"], t1["block"], t1["lds"]) == (2, 1, 4, 512, 512, 32768)
    e1 = by["embed", (128, 256, 16, 16, 768, 1)]
    assert (e1["form"], e1["tpw"], e1["gx"], e1["paths"]) == (1, 6, 1024, 1 << 3)
    assert [LP.cross_row_form(256, G * G, b, 256) for G, b in HG.PARTITION] == [("mfma", 2), ("mfma", 4), ("mfma", 2)]
    a = by["attn", (3, 144, 2)]
    assert (a["form"], a["gx"], a["gy"], a["gz"], a["nbuf"], a["lds"]) == (3, 2, 2, 3, 2, 2 * (128 * 128 + 64 * 264))
    assert by["attn", (3, 16, 2)]["nbuf"] == 1 and by["attn", (3, 128, 2)]["paths"] == 0 == by["attn", (3, 32, 2)]["paths"]


def _cfg(d, G, pd, mult=4):
    C, p = PATCH[pd]
    return NS(image_size=G * p, noise_embed_dims=256, patch_size=p, embed_dim=d, n_layers=2, text_emb_size=768, n_channels=C, mlp_multiplier=mult)


def test_lds_fits_a_cu_wherever_create_accepts(swept):
    """Every form a launch can take at an accepted configuration -- with and without the held images, the hidden activation, the fp8 outputs -- asks for at
    most 160 KiB; the limit binds somewhere (a refused configuration does pass it)."""
    cases, got = swept
    ok = {(d, pd): BP.config_check(_cfg(d, 16, pd), 4) == "" for d in DS for pd in PDS}
    assert not ok[1024, 64] and ok[512, 64] and ok[768, 48] and all(ok[d, 16] and ok[d, 4] for d in DS)
    worst, over = 0, 0
    for (site, args), g in zip(cases, got):
        if site in ("embed", "tail"):
            d, pd = (args[4], args[2]) if site == "embed" else (args[3], args[2])
            accepted = ok[d, pd]
        else:
            accepted = True                                         # (cross_row: every width has an accepted patch; the others do not depend on the configuration)
        if accepted:
            assert 0 <= g["lds"] <= LP.LDS_LIMIT, (site, args, g["lds"])
            worst = max(worst, g["lds"])
        else:
            over += g["lds"] > LP.LDS_LIMIT
    assert worst == LP.LDS_LIMIT == LP.plan_embed(1, 16, 64, 64, 576, 0)["lds"] and over > 0      # (the plain embed at pd 64, d 576 takes exactly the limit)


def _in_reach(site, args, g):
    """x within 2^31 - 1 (a launch over rows has all its workgroups there), y and z within 65 535, and the extents are the count."""
    assert 0 < g["gx"] <= LP.GRID_X and g["gy"] <= LP.GRID_YZ and g["gz"] <= LP.GRID_YZ and g["gx"] * g["gy"] * g["gz"] == g["groups"], (site, args, g)


def test_grid_extents_wherever_create_and_the_hooks_accept(driver, swept):
    for (site, args), g in zip(*swept):
        assert not g.get("refused")
        _in_reach(site, args, g)
    # the engine at the largest max_batch create accepts (bisected on the restatement, which tests/test_body_plan_host.py holds against the header)
    cases = []
    for d, G, mult, pd in itertools.product((64, 192, 256, 768, 1024), (4, 12, 16, 32, 44, 64), (1, 4), (4, 16)):
        cfg = _cfg(d, G, pd, mult)
        lo, hi = 1, 1 << 21
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if "max_batch=" not in BP.config_check(cfg, mid) else (lo, mid - 1)
        assert BP.config_check(cfg, lo) == "" and BP.config_check(cfg, lo + 1)
        b, n, hid = lo, G * G, mult * d
        for cus in CUS:
            cases += [("embed", (b, n, pd, pd, d, 1)), ("ln", (b * n, d, 0)), ("ln", (b * n, d, 1)), ("cross", (b, n, d, d // 64, 0, 0, cus)), ("cross", (b, n, d, d // 64, 1, 1, cus)),
                      ("skf", (b * n, d)), ("tail", (b, n, pd, d, 0, 1, cus)), ("tail", (b, n, pd, d, 1, 1, cus)), ("tail", (b, n, pd, d, 0, 0, cus)), ("dw", (b, G, hid, 0)),
                      ("dw", (b, G, hid, 1)), ("attn", (b, n, d // 64))]
    assert max(args[0] for site, args in cases if site == "attn") == 65535
    for (site, args), g in zip(cases, _plans(driver, cases)):
        assert g == {**LP.PLANS[site](*args), **({"refused": 0} if "refused" in g else {})}, (site, args)
        _in_reach(site, args, g)
    # the two hooks: what they accept is in reach, and they refuse what is not
    hooks = [(("dw", (12000000, 20, 3072, 0)), 1), (("dw", (12000000, 28, 3072, 0)), 1), (("dw", (11000000, 20, 3072, 0)), 0),      # tiled: 4 tiles x 48 chunks per sample
             (("dw", (32768, 32, 64, 0)), 1), (("dw", (32767, 32, 64, 0)), 0),                                                      # streaming: 128 KiB per sample against 4 GiB
             (("dw", (2147483647, 16, 64, 0)), 0), (("dw", (2147483647, 12, 128, 0)), 1),                                             # whole image: one workgroup per chunk
             (("attn", (65535, 144, 2)), 0), (("attn", (65536, 144, 2)), 1), (("attn", (3, 64, 65536)), 1), (("attn", (65536, 256, 2)), 1),      # samples on z, heads on y
             (("attn", (70000, 512, 2)), 0), (("attn", (2147483647, 512, 1)), 1), (("attn", (2147483647, 4096, 16)), 1),              # chunked: everything on x
             (("attn", (8388607, 4096, 16)), 0), (("attn", (8388608, 4096, 16)), 1)]
    res = _plans(driver, [h for h, _ in hooks])
    for ((site, args), refused), g in zip(hooks, res):
        assert {k: v for k, v in g.items() if k != "refused"} == LP.PLANS[site](*args), (site, args)
        assert g["refused"] == refused, (site, args, g)
        if not refused:
            _in_reach(site, args, g)
        else:
            assert g["groups"] > LP.GRID_X or g["gy"] > LP.GRID_YZ or g["gz"] > LP.GRID_YZ or (site == "dw" and g["form"] == 2), (site, args, g)


def _engine_line(name, d, G, L, max_batch, fp8=False, fused=True):
    cfg = NS(**{k: v for k, v in FS._cfg(d, 2 * G, L).items() if k != "dropout"})
    return TB._line(name, cfg, max_batch, "d1" if fp8 else "-", {} if fused else {"TLD_FP8_FUSED": "0"}, HG.CUS_MI355X)


def test_paths_of_the_plans_are_what_the_grid_tests_expect(body_driver):
    """The whole ENGINE, PARTITION and SAMPLER_GRIDS tables of tests/test_forward_grids_host.py: every bit a plan sets is a bit expected_paths wants set, every bit it
    wants set that a row or attention launch owns is set, and no bit it wants clear is set."""
    rows = []
    for fam, d, G, b, fp8 in HG.ENGINE:
        for fused in ((True, False) if fp8 else (True,)):
            rows.append((_engine_line(f"{fam}g{G}", d, G, 2, b, fp8, fused), 3, HG.expected_paths(d, G, b, HG.CUS_MI355X, fp8=fp8, fp8_fused=fused)))
    rows += [(_engine_line(f"part{G}x{b}", 256, G, 1, b), 3, HG.expected_paths(256, G, b, HG.CUS_MI355X)) for G, b in HG.PARTITION]
    rows += [(_engine_line(f"s{G}", 256, G, 2, 2 * HG.SAMPLER_B), 4, HG.expected_paths(256, G, 2 * HG.SAMPLER_B, HG.CUS_MI355X, sampler=True)) for G in HG.SAMPLER_GRIDS]
    assert len(rows) == len(HG.ENGINE) + 6 + 3 + 3
    for o, (line, k, (on, off)) in zip(body_driver([r[0] for r in rows]), rows):
        assert o["create"] == "", line
        mask = o["launch"][k]
        have = {b for b in range(64) if mask >> b & 1}
        assert have <= LP.OWNED and have == on & LP.OWNED and not have & off, (line, sorted(have), sorted(on & LP.OWNED), sorted(have & off))


def test_no_plan_of_the_body_sweep_meets_a_width_without_its_kernel(body_driver):
    """plan_layernorm, plan_cross_row and plan_splitk_finish answer "no such kernel / no such output" at some widths.  Over the whole sweep of
    tests/test_body_plan_host.py -- every configuration the GPU stage tests and the golden sweep run, every switch, both operand types, every class, both CU counts -- a
    plan that sets ln_mx8, fold_ln3 or cross_mx8, or ll_split never meets that answer: the launchers' branch for it is unreachable from the engine."""
    cases = list(TB._sweep())
    asked = [0, 0, 0]
    for o, case in zip(body_driver([TB._line(name, cfg, mb, ops, env, cus) for name, cfg, mb, env, ops, cus in cases]), cases):
        p, (ln, cross, skf, _, _) = o["plan"], o["launch"]
        assert (ln == LP.LN_FORMS.index("mx8")) if p["ln_mx8"] else ln == -1, case
        assert (cross == 1) if p["fold_ln3"] or p["cross_mx8"] else cross == -1, case
        assert (skf in (1, 2)) if p["ll_split"] else skf == -1, case
        asked = [a + (v != -1) for a, v in zip(asked, (ln, cross, skf))]
    assert all(asked), asked
    # ... and the answer exists: the widths the three predicates of the mode turn down
    assert [d for d in DS if LP.plan_layernorm(4, d, True)["form"]] == [256, 512, 768] == [d for d in DS if LP.plan_cross_row(1, 16, d, d // 64, 0, 0, 256)["mode_outputs"]]
    assert [d for d in DS if LP.plan_splitk_finish(4, d)["form"]] == [384, 768]

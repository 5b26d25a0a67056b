"""CPU: the host decisions of the training step -- csrc/tld_train_plan.h through tests/host/train_plan_main.cpp, built by the host
compiler plain and under AddressSanitizer + UBSan, against the restatement in tests/train_plan_ref.py (which keeps the weight-gradient split as the two loops
and the power-of-two loop the engine had); and the invariants the engine cannot check itself: every site's partial-sum demand at every batch fits what
tld_train_create allocates, every chosen split fits its slice and operand workspace, tall_dw's capacity condition never decides, and the predicted mask has
one bit in each exclusive group of the table in include/tld_hip.h (the weight-gradient bits, chosen per product, one of the sets a step can show)."""
import itertools
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import pytest

import test_gpu_large_offsets as LO
import test_gpu_train as TG
import test_gpu_train_stages as TS
import train_plan_ref as P
from conftest import cfg_from_arr, load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("image_size", "noise_embed_dims", "patch_size", "embed_dim", "n_layers", "text_emb_size", "n_channels", "mlp_multiplier")


def _cfg(d=128, image=16, blocks=3, patch=2, C=4, mult=4, ne=256, text=768):      # (the defaults of DenoiserConfig)
    return NS(image_size=image, noise_embed_dims=ne, patch_size=patch, embed_dim=d, n_layers=blocks, text_emb_size=text, n_channels=C, mlp_multiplier=mult)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver, built twice (run directly, nothing preloaded); ``run(lines)`` returns the parsed output, the same from both builds."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    tmp = tmp_path_factory.mktemp("train_plan")
    src = [os.path.join(REPO, "tests", "host", "train_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"train_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exes[tag]], check=True)

    def run(lines):
        path = tmp / f"cases_{len(os.listdir(tmp))}.txt"
        path.write_text("".join(ln + "\n" for ln in lines))
        outs = []
        for tag, exe in exes.items():
            r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
            outs.append(r.stdout)
        assert outs[0] == outs[1], "the sanitizer build answers differently"
        res = [json.loads(ln) for ln in outs[0].splitlines()]
        assert len(res) == len(lines)
        return res

    return run


# ---- the sweep: every configuration a GPU test creates a trainer at ---------------------------------------------------------------------------------------------
def _configs():
    """name -> (config, the test's batch, max_batch)"""
    out = {}
    for name, (kw, batch, max_batch) in TS.CASES.items():
        out["stages " + name] = (NS(**kw), batch, max_batch)
    from transformer_latent_diffusion_amd import DenoiserConfig
    for name in TG.GOLDEN_STEPS:                                              # tests/test_gpu_train.py: its two golden steps and its table of shapes
        g = load_golden(name)
        out["train " + name[:3]] = (cfg_from_arr(g["cfg"]), int(g["x"].shape[0]), 4)
    for name, (kw, batch, max_batch) in TG.TRAINER_SHAPES.items():
        out["train " + name] = (DenoiserConfig(**kw), batch, max_batch)
    for name, (kw, max_batch) in LO.TRAINERS.items():                        # tests/test_gpu_large_offsets.py
        out["large " + name] = (NS(**kw), max_batch, max_batch)
    return out


def _line(cfg, max_batch, batch, cus, tn):
    return " ".join(["plan", *(str(getattr(cfg, f)) for f in FIELDS), str(max_batch), str(batch), str(cus), str(int(tn))])


def _sweep():
    for (name, (cfg, batch, mb)), cus, tn in itertools.product(_configs().items(), (256, 304), (0, 1)):
        for b in sorted({1, batch, mb}):
            yield name, cfg, mb, b, cus, tn


def _check(o, cfg, mb, b, cus, tn):
    """One plan line against the restatement, then the invariants."""
    assert o["refusal"] == ""
    sh = P.shape(cfg, mb)
    ws = P.workspace(sh)
    assert o["shape"] == vars(sh) and o["workspace"] == vars(ws)
    ref, demands = P.step_plan(sh, ws, b, cus, bool(tn))
    assert o["plan"] == vars(ref), (o["plan"], vars(ref))
    assert o["demands"] == demands
    # every site's demand, at every batch 1 .. max_batch, fits the partial-sum buffer
    assert o["fits"]["largest_demand"] <= ws.part_floats, (o["fits"], ws.part_floats)
    assert max(f for _, f in o["demands"]) <= o["fits"]["largest_demand"] or b > mb
    # every chosen split fits its slices; a transposing one its operand rows
    for (form, sk, rows), (nout, kin) in zip(o["plan"]["wg"], ((sh.d, sh.hid), (sh.hid, sh.d), (sh.d, sh.d), (3 * sh.d, sh.d))):
        assert sk * nout * kin <= ws.splitk_floats, (form, sk, nout, kin)
        assert form == P.WG_TN or sk * rows <= ws.tr_rows, (form, sk, rows)
        assert sk * rows >= o["plan"]["M"] and (sk - 1) * rows < o["plan"]["M"] and rows % 64 == 0
    # tall_dw's capacity condition never selects the fallback where the column kernel exists
    for nn, K, _ in o["plan"]["tall"]:
        assert nn == (sh.pd if sh.pd in (16, 32, 64) else 0), (nn, sh.pd)
    # exactly one bit in each exclusive group
    for group, bits in P.EXCLUSIVE.items():
        assert sum(o["plan"]["paths"] >> k & 1 for k in bits) == 1, (group, hex(o["plan"]["paths"]))
    assert {k for k in range(24, 28) if o["plan"]["paths"] >> k & 1} in P.WGRAD_SETS, hex(o["plan"]["paths"])


def test_sweep_against_the_restatement_and_invariants(driver):
    cases = list(_sweep())
    assert len(_configs()) == len(TS.CASES) + len(TG.GOLDEN_STEPS) + len(TG.TRAINER_SHAPES) + len(LO.TRAINERS) and {c[0] for c in cases} >= {"stages " + n for n in TS.TN_OFF_CASES}
    outs = driver([_line(cfg, mb, b, cus, tn) for _, cfg, mb, b, cus, tn in cases])
    masks = 0
    for o, (name, cfg, mb, b, cus, tn) in zip(outs, cases):
        _check(o, cfg, mb, b, cus, tn)
        masks |= o["plan"]["paths"]
    assert masks == (1 << 31) - 1, hex(masks)          # the sweep predicts every launch path


def test_part_demand_at_every_accepted_shape(driver):
    """Beyond the swept configurations: every width, grid and patch the trainer accepts, at a small and an odd max_batch -- the partial-sum buffer holds every
    site's demand at every batch, and the column form of tall_dw is never refused for capacity."""
    cases = []
    for d, (image, patch, C), mult, mb in itertools.product(range(64, 1025, 64), ((8, 2, 4), (16, 2, 4), (24, 2, 4), (32, 2, 4), (64, 2, 4), (64, 4, 4), (32, 2, 3), (40, 2, 8), (16, 1, 3), (128, 2, 4)),
                                                           (1, 2, 4), (1, 3, 37)):
        cases.append((_cfg(d=d, image=image, patch=patch, C=C, mult=mult, blocks=1), mb))
    outs = driver([_line(cfg, mb, mb, 256, 1) for cfg, mb in cases])
    seen_both = 0
    for o, (cfg, mb) in zip(outs, cases):
        assert o["refusal"] == "", (vars(cfg), o["refusal"])
        sh = P.shape(cfg, mb)
        assert o["fits"]["largest_demand"] <= o["workspace"]["part_floats"], (vars(cfg), mb, o["fits"])
        assert all(nn == (sh.pd if sh.pd in (16, 32, 64) else 0) for nn, _, _ in o["plan"]["tall"])
        # the mask, here too: the restatement's, one bit per group -- but BOTH column-sum bits where patch_dim is no multiple of 4 at 4096 rows or more
        # (C = 3, patch 1: the bias sums of width 3 take colsum_partial, those of width d colsum4_partial)
        mask = o["plan"]["paths"]
        assert mask == P.expected_mask(vars(cfg), mb, mb, 256, 1)
        both = sh.pd % 4 != 0 and mb * sh.N >= 4096
        seen_both += both
        for group, bits in P.EXCLUSIVE.items():
            assert sum(mask >> k & 1 for k in bits) == (2 if group == "colsum" and both else 1), (vars(cfg), mb, group, hex(mask))
        assert {k for k in range(24, 28) if mask >> k & 1} in P.WGRAD_SETS
    assert seen_both


# ---- the chooser alone ------------------------------------------------------------------------------------------------------------------------------------------
def test_dense_sweep_of_the_split_against_the_two_loops(driver):
    """M over every multiple of 16 up to 40 000, the four products of d in {256, 512, 768, 1024} at multiplier 4, 256 and 304 CUs, with the workspace of an
    engine whose max_batch has exactly those rows: the one chooser returns what the untransposed loop, the transposing loop and the power-of-two loop returned.
    Also where the power-of-two loop still decides, so that it stays in the chooser."""
    cases = []
    for d in (256, 512, 768, 1024):
        hid = 4 * d
        for nout, kin in ((d, hid), (hid, d), (d, d), (3 * d, d)):
            for cus in (256, 304):
                cases += [(M, nout, kin, cus, 8 * hid * d, M + P.TRANSPOSE_MARGIN) for M in range(16, 40001, 16)]
    outs = driver([f"wgrad {M} {a} {b} {cus} {sl} {tr}" for M, a, b, cus, sl, tr in cases])
    pow2_decides = []
    for o, (M, a, b, cus, sl, tr) in zip(outs, cases):
        assert tuple(o["tn"]) == P.wgrad(M, a, b, cus, True, sl, tr), (M, a, b, cus, o)
        assert tuple(o["tr"]) == P.wgrad(M, a, b, cus, False, sl, tr), (M, a, b, cus, o)
        if o["tr"][1] > 1 and M < 4096:
            pow2_decides.append((M, a, b))
    # the power-of-two loop decides an outcome (2048 <= M < 4096, M a multiple of 256): it cannot leave the chooser.  The smallest such shape:
    assert min(pow2_decides) == (2048, 256, 256) and all(M % 256 == 0 for M, _, _ in pow2_decides)


def test_the_recorded_splits_of_case_a(driver):
    """Computed from the engine's loops before they moved: case A (d 768, M 32 768) at 256 CUs, up / down at 304 CUs, and the zero-padded cases B and F."""
    d, hid, M = 768, 3072, 32768
    sl, tr = 8 * hid * d, M + P.TRANSPOSE_MARGIN
    lines = [f"wgrad {M} {a} {b} {cus} {sl} {tr}" for a, b, cus in ((hid, d, 256), (d, hid, 256), (3 * d, d, 256), (d, d, 256), (hid, d, 304), (d, hid, 304))]
    up, down, qkv, q, up304, down304 = driver(lines)
    assert up["tn"] == down["tn"] == [P.WG_TN, 7, 4736] and up["tr"] == down["tr"] == [P.WG_TRSK, 7, 4736]
    assert qkv["tn"] == [P.WG_TN, 9, 3648] and qkv["tr"] == [P.WG_TRSK, 9, 3712]
    assert q["tn"] == [P.WG_TN, 27, 1216] and q["tr"] == [P.WG_TRSK, 26, 1280]
    assert up304["tn"] == down304["tn"] == [P.WG_TN, 8, 4096]
    # the smallest shape at which the two rules answer differently for one product with the same capacities, and the one before it
    a, b = driver([f"wgrad {M} 256 1024 256 {8 * 1024 * 256} {M + P.TRANSPOSE_MARGIN}" for M in (1984, 1920)])
    assert a == {"tn": [P.WG_TN, 2, 1024], "tr": [P.WG_TR1, 1, 1984]} and b["tn"][1:] == b["tr"][1:] == [1, 1920]
    for case, rows in (("B", 448), ("F", 832)):
        kw, batch, mb = TS.CASES[case]
        for tn in (0, 1):
            o, = driver([_line(NS(**kw), mb, batch, 256, tn)])
            assert o["plan"]["wg"] == [[P.WG_PAD, 1, rows]] * 4, (case, o["plan"]["wg"])


def test_attention_backward_dispatch(driver):
    """attn_bwd_dispatch against the restatement tests/test_gpu_attn_bwd_classes.py builds its case tables from, at every multiple of 16 up to 4096 and at the
    counts it refuses.  64, 128 and 256 tokens take the exact 2-, 4- and 8-wave single-workgroup kernels by the general rule."""
    ns = list(range(16, 4097, 16)) + [0, -16, 8, 24, 250, 4100]
    outs = driver([f"attn {n} {hs}" for n in ns for hs in (1, 0)])
    for k, n in enumerate(ns):
        for j, hs in enumerate((1, 0)):
            o = outs[2 * k + j]
            mode, nw, masked = P.attn_dispatch(n, bool(hs))
            assert (o["mode"], o["waves"], o["masked"]) == (mode, nw, int(masked)), (n, hs, o)
            assert o["path"] == (mode | (4 if masked else 0))
    by = {n: outs[2 * k] for k, n in enumerate(ns)}
    assert [(by[n]["mode"], by[n]["waves"], by[n]["masked"]) for n in (64, 128, 256)] == [(1, 2, 0), (1, 4, 0), (1, 8, 0)]
    assert by[256] == outs[2 * ns.index(256) + 1] and outs[2 * ns.index(272) + 1]["mode"] == 0          # no scratch: 256 tokens still run, 272 are refused


def test_expected_mask_is_the_plan_of_the_driver(driver):
    """expected_mask, which tests/test_gpu_train_stages.py holds every case's recorded mask against, is the driver's prediction."""
    rows = [(NS(**kw), batch, mb, cus, tn) for (kw, batch, mb) in TS.CASES.values() for cus in (256, 304) for tn in (0, 1)]
    outs = driver([_line(cfg, mb, b, cus, tn) for cfg, b, mb, cus, tn in rows])
    for o, (cfg, b, mb, cus, tn) in zip(outs, rows):
        assert o["plan"]["paths"] == P.expected_mask(vars(cfg), b, mb, cus, tn)

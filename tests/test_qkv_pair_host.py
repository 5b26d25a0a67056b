"""CPU: the host side of the two-head form of the fused QKV + attention kernel (EPI_QKV_ATTN2) -- the row order of its weight image
(csrc/tld_refresh_math.h: qkv_pair_row) against a numpy statement of the tile layout, and the selection rule (csrc/tld_qkv_pair_plan.h: plan_qkv_pair)
through tests/host/qkv_pair_main.cpp (plain and under AddressSanitizer + UBSan, run directly) and through the library's debug export."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS, CUS, SAMPLES = (6, 12, 16), (256, 304), range(1, 513)


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    out = tmp_path_factory.mktemp("qkv_pair")
    src = [os.path.join(REPO, "tests", "host", "qkv_pair_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = []
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(out / f"qkv_pair_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exe], check=True)
        exes.append(exe)
    return exes


def _run(exe, *args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (exe, args, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def pair_rows(d):
    """Pair-ordered row of every row n = part * d + head * 64 + feature of the [3 d][d] QKV weight, from the layout sentence: a 256 x 384 tile is the head
    pair p; its column c = [quarter wn = c / 96][part (c % 96) / 32: q | k | v][side (c % 32) / 16: head A | B][16 features], feature 16 wn + c % 16."""
    R = np.arange(3 * d)
    p, c = R // 384, R % 384
    wn, part, side, feat = c // 96, (c % 96) // 32, (c % 32) // 16, 16 * (c // 96) + c % 16
    src = part * d + (2 * p + side) * 64 + feat          # the original row that pair-ordered row R holds
    out = np.full(3 * d, -1)
    out[src] = R
    return out, (p, wn, part, side, feat)


@pytest.mark.parametrize("d", [384, 768])
def test_pair_row_map_is_the_tile_layout(mains, d):
    want, (p, wn, part, side, feat) = pair_rows(d)
    assert sorted(want) == list(range(3 * d))                                  # a bijection of [0, 3 d)
    for exe in mains:
        got = np.array(_run(exe, "rows", str(d)).split(), dtype=np.int64)
        assert np.array_equal(got, want), (exe, np.flatnonzero(got != want)[:8])
    # every 96-column wave group holds 16 features x {q, k, v} x {head A, head B}, and all of them of the same two heads
    for g in range(3 * d // 96):
        sl = slice(96 * g, 96 * g + 96)
        assert len(set(p[sl])) == 1 and len(set(wn[sl])) == 1
        cells = set(zip(part[sl], side[sl], feat[sl] - 16 * wn[sl]))
        assert cells == {(a, b, f) for a in range(3) for b in range(2) for f in range(16)}


def _stated_rule(samples, heads, cus, num, den):
    if heads % 2:
        return False
    items = samples * heads
    return math.ceil(items // 2 / cus) * num < math.ceil(items / cus) * den      # ceil(pairs / CUs) t_pair < ceil(items / CUs) t_item


def test_selection_follows_the_stated_inequality(mains):
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    q = np.array([(s, h, c) for h in HEADS for c in CUS for s in SAMPLES], dtype=np.int32)
    got = np.zeros(len(q), dtype=np.int32)
    ratio = np.zeros(2, dtype=np.int32)
    _lib.check(L.tld_debug_qkv_pair_plan(q.ctypes.data, len(q), got.ctypes.data, ratio.ctypes.data), "tld_debug_qkv_pair_plan")
    num, den = int(ratio[0]), int(ratio[1])
    assert den > 0 and 1.0 < num / den < 2.0, (num, den)       # a two-head tile costs more than one item and less than two, or the form has no reason to exist
    want = np.array([_stated_rule(int(s), int(h), int(c), num, den) for s, h, c in q], dtype=np.int32)
    assert np.array_equal(got, want), q[got != want][:8]
    for exe in mains:                                        # the stand-alone driver says the same
        lines = _run(exe, "plan").split("\n")
        assert lines[0] == f"ratio {num} {den}"
        table = "".join(ln.split()[2] for ln in lines[1:] if ln)
        assert table == "".join(map(str, got)), exe
    plan = {(int(s), int(h), int(c)): bool(g) for (s, h, c), g in zip(q, got)}
    assert plan[(128, 12, 256)]                              # C1's blocks 1 - 11: 768 pairs = 3 whole rounds
    assert not plan[(64, 12, 256)]                           # C1's block 0 on the shared half batch: 1.5 rounds of pairs against 3 of items
    assert not plan[(2, 12, 256)] and not plan[(1, 16, 304)]
    one = np.array([(s, h, 256) for h in (1, 3, 5, 7, 9) for s in SAMPLES], dtype=np.int32)      # never a pair form for odd heads
    res = np.ones(len(one), dtype=np.int32)
    _lib.check(L.tld_debug_qkv_pair_plan(one.ctypes.data, len(one), res.ctypes.data, None), "tld_debug_qkv_pair_plan")
    assert not res.any()

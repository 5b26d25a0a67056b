"""CPU: which kernel every GEMM launch gets -- plan_gemm (csrc/tld_gemm_plan.h) through tld_debug_gemm_plan, host arithmetic only.

Three layers: a frozen table of plans recorded from the selection code this function replaced (tests/golden/g20_gemm_plans.npz, see tests/golden/README.md);
the named shapes of the benchmark configurations, each with the sentence that motivates its plan; and the invariants the kernels' numerics and
schedules rely on, asserted over the whole sweep."""
import hashlib

import numpy as np
import pytest

from conftest import load_golden
from transformer_latent_diffusion_amd import _lib

# GemmEpilogue (csrc/tld_gemm_params.h)
EPI_F32, EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID, EPI_UP_DWCONV32, EPI_QKV_LN, EPI_UP_DWCONV2, EPI_QKV_ATTN = range(8)
EPILOGUES = tuple(range(8))
# query columns (include/tld_hip.h)
Q = {n: i for i, n in enumerate(("M", "N", "K", "lda", "ldw", "ldo", "ldr", "epilogue", "f8", "conv", "cv_cin", "cv_up", "cv_down", "ksplit", "w_batch_rows",
                                 "has_bias", "has_resid", "has_c_f32", "ncu", "f8_ring", "half_tail", "updw_small", "splitk_small", "down_small"))}
SWITCHES = ("f8_ring", "half_tail", "updw_small", "splitk_small", "down_small")
# plan columns
FAMILY, BN, BM, RING, XCD, HALF_TAIL, NBLOCKS, BLOCK, REFUSAL = range(9)
REFUSED, MAIN, UPDW_PP, SPLITK_PP, DOWN_PP = range(5)

# ---- the sweep ---------------------------------------------------------------------------------------------------------------------------------------------
IMAGES = (1, 2, 3, 4, 5, 6, 7, 8, 16, 64, 128)
TOKENS = (256, 1024, 4096)           # per image at 256 / 512 / 1024 px (C1, C3, C4)
# rows of a launch: the CFG pair of every image (2 i tokens) and block 0 of the shared-conditioning path, which runs on the un-doubled batch (i tokens)
M_MODEL = sorted({f * i * t for f in (1, 2) for i in IMAGES for t in TOKENS})
M_OTHER = (64, 128, 192, 320, 384, 448, 576, 640, 1000, 1280, 2560, 5000, 16640, 20000, 49152)      # multiples of 64 that are not multiples of 256, and non-multiples of 64
MS = sorted(set(M_MODEL) | set(M_OTHER))
NS = (128, 192, 256, 384, 512, 768, 1024, 1152, 1536, 2304, 3072, 4608)
KS_CONV = (9 * 64, 9 * 128, 9 * 192, 9 * 512)
KS = (64, 128, 192, 256, 384, 768, 3072) + KS_CONV
MODES = ("bf16", "fp8", "conv", "splitk2", "splitk4", "splitk8")
EPILOGUES_SWEPT = EPILOGUES + (8,)      # 8: not an epilogue
ALL_ON = (1, 1, 1, 1, 1)
# (CU count, switches): every switch on and off at 256 CUs (MI355X) and at 304 (8 XCDs x 38: what the hard-coded 256 / 8 / 32 of the tile-width rules do off this part);
# 60 CUs: not a multiple of 8, no XCD groups
VARIANTS = [(ncu, tuple(0 if j == off else 1 for j in range(5))) for ncu in (256, 304) for off in (None, 0, 1, 2, 3, 4)] + [(60, ALL_ON)]


def _rows(**cols):
    """Cartesian product of the given columns (sequences) over the defaults of a plain bf16 launch; returns int32 [n][24]."""
    names = list(cols)
    grids = np.meshgrid(*[np.asarray(cols[n], np.int64) for n in names], indexing="ij")
    n = grids[0].size
    q = np.zeros((n, len(Q)), np.int64)
    q[:, Q["has_bias"]] = q[:, Q["has_resid"]] = q[:, Q["has_c_f32"]] = 1
    q[:, Q["ksplit"]] = 1
    for name, g in zip(names, grids):
        q[:, Q[name]] = g.reshape(-1)
    return q


def _finish(q, ncu, switches):
    """Pitches as the callers set them: K-contiguous operands (split-K: K is ONE split of the row), dense outputs."""
    q = q.copy()
    for c in ("lda", "ldw"):
        unset = q[:, Q[c]] == 0
        q[unset, Q[c]] = (q[:, Q["K"]] * np.maximum(q[:, Q["ksplit"]], 1))[unset]
    for c in ("ldo", "ldr"):
        unset = q[:, Q[c]] == 0
        q[unset, Q[c]] = q[unset, Q["N"]]
    q[:, Q["cv_cin"]] = np.where(q[:, Q["conv"]] != 0, q[:, Q["K"]] // 9, 0)
    q[:, Q["ncu"]] = ncu
    for j, s in enumerate(SWITCHES):
        q[:, Q[s]] = switches[j]
    return q.astype(np.int32)


def sweep_chunk(ncu, switches):
    """All query rows of one (CU count, switches) variant."""
    parts = []
    for mode in MODES:
        kw = dict(epilogue=EPILOGUES_SWEPT, M=MS, N=NS, K=KS_CONV if mode == "conv" else KS)
        if mode == "fp8":
            kw["f8"] = (1,)
        elif mode == "conv":
            kw["conv"] = (1,)
        elif mode.startswith("splitk"):
            kw["ksplit"] = (int(mode[6:]),)
        parts.append(_rows(**kw))
    small_m, some_n, some_k = (256, 512, 2048, 4096, 65536), (384, 768, 3072), (256, 768, 3072)
    # operands the small-batch forms need, absent one at a time; pitches they cannot take; block-diagonal W; the two conv addressing modes and both at once
    for absent in ("has_bias", "has_resid", "has_c_f32"):
        parts.append(_rows(epilogue=(EPI_F32, EPI_BIAS_RESID), M=small_m, N=some_n, K=some_k, ksplit=(1, 4), **{absent: (0,)}))
    parts.append(_rows(epilogue=(EPI_BIAS_RESID, EPI_UP_DWCONV2), M=small_m, N=some_n, K=some_k, ldo=(770, 3074), ldr=(770, 3074)))
    parts.append(_rows(epilogue=(EPI_F32, EPI_BIAS_RESID, EPI_UP_DWCONV2), M=small_m, N=some_n, K=some_k, ksplit=(1, 4), lda=(1 << 23, 32768), ldw=(1 << 23, 32768)))
    parts.append(_rows(epilogue=EPILOGUES, M=small_m, N=some_n, K=some_k, ksplit=(1, 4), w_batch_rows=(256,)))
    parts.append(_rows(epilogue=EPILOGUES, M=small_m + (49152,), N=(128, 256, 512), K=KS_CONV, conv=(1,), cv_up=(0, 1), cv_down=(0, 1)))
    return _finish(np.concatenate(parts), ncu, switches)


def plans_of(q):
    q = np.ascontiguousarray(q, np.int32).reshape(-1, len(Q))
    out = np.zeros((len(q), 9), np.int32)
    _lib.check(_lib.lib().tld_debug_gemm_plan(q.ctypes.data, len(q), out.ctypes.data), "tld_debug_gemm_plan")
    return out


def plan(M, N, K, epilogue, ncu=256, switches=ALL_ON, **kw):
    return plans_of(_finish(_rows(M=(M,), N=(N,), K=(K,), epilogue=(epilogue,), **{k: (v,) for k, v in kw.items()}), ncu, switches))[0]


@pytest.fixture(scope="module")
def sweep():
    """[(queries, plans)] per variant, from the function under test."""
    return [(q, plans_of(q)) for q in (sweep_chunk(ncu, sw) for ncu, sw in VARIANTS)]


# ---- 1. the frozen table ------------------------------------------------------------------------------------------------------------------------------------
def test_every_plan_equals_the_frozen_table(sweep):
    """Every field of every row.  The table holds, per variant, the SHA-256 of the query rows it was recorded for and the recorded plans as indices into the list of distinct plans."""
    g = load_golden("g20_gemm_plans.npz")
    assert [tuple(v) for v in g["variants"]] == [(ncu,) + sw for ncu, sw in VARIANTS]
    distinct = g["distinct_plans"]
    offsets = g["offsets"]
    for i, (q, got) in enumerate(sweep):
        assert hashlib.sha256(q.tobytes()).hexdigest() == str(g["query_sha256"][i]), f"variant {VARIANTS[i]}: the sweep is not the one the table was recorded for"
        want = distinct[g["plan_index"][offsets[i]:offsets[i + 1]]]
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, (f"variant {VARIANTS[i]}: {bad.size} of {len(q)} plans differ from the table; first: query "
                               f"{dict(zip(Q, q[bad[0]].tolist()))} -> {got[bad[0]].tolist()}, recorded {want[bad[0]].tolist()}")


def test_refusals_of_combinations_without_a_kernel(sweep):
    """Epilogue / operand-mode combinations no kernel is instantiated for are refused with a reason (they used to launch nothing and report success)."""
    for q, p in sweep:
        epi, f8, conv = q[:, Q["epilogue"]], q[:, Q["f8"]] != 0, q[:, Q["conv"]] != 0
        both = conv & (q[:, Q["cv_up"]] != 0) & (q[:, Q["cv_down"]] != 0)
        no_kernel = (epi == 8) | (conv & ~np.isin(epi, (EPI_F32, EPI_BIAS_BF16, EPI_BIAS_RESID))) | (f8 & ~conv & ~np.isin(epi, (EPI_F32, EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID)))
        assert (p[both, FAMILY] == REFUSED).all() and (p[both, REFUSAL] == 1).all()
        assert (p[no_kernel & ~both, FAMILY] == REFUSED).all() and (p[no_kernel & ~both, REFUSAL] == 2).all()
        assert (p[~no_kernel & ~both, FAMILY] != REFUSED).all() and (p[p[:, FAMILY] != REFUSED, REFUSAL] == 0).all()
        assert (p[p[:, FAMILY] == REFUSED][:, [BN, BM, RING, XCD, HALF_TAIL, NBLOCKS, BLOCK]] == 0).all()


# ---- 2. named shapes ---------------------------------------------------------------------------------------------------------------------------------------
def test_c1_down_projection_is_one_round_of_384_wide_tiles():
    """'down projection at the bench size: 256 x 384 tiles make N = 768 ONE round of 256 workgroups (176 -> 155 us)' (tld_gemm_plan.h)."""
    p = plan(32768, 768, 3072, EPI_BIAS_RESID)
    assert (p[FAMILY], p[BN], p[RING], p[NBLOCKS], p[BLOCK]) == (MAIN, 384, 0, 256, 512)
    # 'any other batch size of that width uses 192-wide tiles, never 128 / 256' -- e.g. 70 samples
    assert plan(70 * 256, 768, 3072, EPI_BIAS_RESID)[BN] == 192


def test_c3_block0_qkv_is_256_wide_with_the_half_tile_tail():
    """'256-wide tiles then beat twice as many 128-wide ones (C3's block-0 QKV projection, 16 384 rows x 2304: 576 tiles = 2.25 rounds; 84 us as 1152 tiles of 128)'."""
    for epi in (EPI_QKV, EPI_QKV_LN):
        p = plan(16384, 2304, 768, epi)
        assert (p[FAMILY], p[BN], p[RING], p[HALF_TAIL], p[XCD], p[NBLOCKS]) == (MAIN, 256, 1, 1, 0, 256)
    # TLD_GEMM_HALFTAIL=0: the width rule does not look at the switch, so the launch keeps its 256-wide tiles with a quarter-full last round and no row split
    # (recorded here as it is; fixing it changes this line and the frozen table)
    p = plan(16384, 2304, 768, EPI_QKV_LN, switches=(1, 0, 1, 1, 1))
    assert (p[FAMILY], p[BN], p[RING], p[HALF_TAIL]) == (MAIN, 256, 1, 0)
    # without the tail rule the same launch is narrow: K = 192 is no whole number of ring iterations
    assert plan(16384, 2304, 192, EPI_QKV_LN)[BN] == 128


def test_vae_attention_projection_at_128_channels_is_128_wide():
    """'The VAE's attention projection at 128 channels and 65 536 tokens -- N = 384, K = 128, 256 tile-rows -- met the other conditions [of the 384-wide bias tile] and came
    out wrong in every row; it takes the 128-wide tiles like every other K = 128 launch.'"""
    p = plan(65536, 384, 128, EPI_BIAS_BF16)
    assert (p[FAMILY], p[BN], p[RING]) == (MAIN, 128, 0)
    # the shape the 384-wide bias tile was built for: the training step's N = 768 linears at batch 128
    assert plan(32768, 768, 768, EPI_BIAS_BF16)[BN] == 384 and plan(32768, 768, 3072, EPI_BIAS_BF16)[BN] == 384


def test_c4_fp8_down_projection_is_256_wide():
    """'where 256-wide tiles fill whole rounds they beat the 192-wide ones -- the down projection at C4, 65 536 rows: 768 tiles in 3 rounds against 1024 in 4, 207.7 -> 174.8 us'."""
    p = plan(65536, 768, 3072, EPI_BIAS_RESID, f8=1)
    assert (p[FAMILY], p[BN], p[RING], p[NBLOCKS]) == (MAIN, 256, 0, 256)         # (fp8 + residual add: the two-stage loop)
    assert plan(32768, 768, 3072, EPI_BIAS_RESID, f8=1)[BN] == 192                # 384 tiles of 256 are 1.5 rounds; 512 of 192 are two whole ones


def test_one_image_at_c1_takes_the_small_batch_forms():
    """'one to five images per call: one 256 x 128 tile per workgroup on twice as many CUs finishes sooner than one 256 x 256 tile (17.7 vs 28.6 us at one image)'; the default
    class's down projection on 64-row tiles 'while they fit' one per CU; the low-latency classes' split-K down projection 'at most TWO items per CU'."""
    M = 2 * 256                                                  # the CFG pair of one image
    assert plan(M, 3072, 768, EPI_UP_DWCONV2)[[FAMILY, BN, BM, NBLOCKS, BLOCK]].tolist() == [UPDW_PP, 128, 256, 48, 256]
    assert plan(M, 768, 3072, EPI_BIAS_RESID)[[FAMILY, BN, BM, NBLOCKS, BLOCK]].tolist() == [DOWN_PP, 192, 64, 32, 256]
    assert plan(M, 768, 768, EPI_F32, ksplit=4)[[FAMILY, BN, BM, NBLOCKS, BLOCK]].tolist() == [SPLITK_PP, 128, 256, 48, 256]      # class 1: four K-splits
    assert plan(M, 768, 384, EPI_F32, ksplit=8)[[FAMILY, BN, BM, NBLOCKS, BLOCK]].tolist() == [SPLITK_PP, 128, 256, 96, 256]      # class 2: eight
    # the switches the subprocess tests set select the 8-wave kernels instead
    assert plan(M, 3072, 768, EPI_UP_DWCONV2, switches=(1, 1, 0, 1, 1))[[FAMILY, BN, RING]].tolist() == [MAIN, 256, 1]
    assert plan(M, 768, 768, EPI_F32, ksplit=4, switches=(1, 1, 1, 0, 1))[[FAMILY, BN, RING, NBLOCKS]].tolist() == [MAIN, 128, 0, 48]
    assert plan(M, 768, 3072, EPI_BIAS_RESID, switches=(1, 1, 1, 1, 0))[[FAMILY, BN]].tolist() == [MAIN, 192]
    # six images: 288 tiles of 256 x 128 are more than one per CU
    assert plan(6 * M, 3072, 768, EPI_UP_DWCONV2)[FAMILY] == MAIN


# ---- 3. invariants over the whole sweep ---------------------------------------------------------------------------------------------------------------------
def _instantiated(bn, epi, f8, conv):
    """The kernels the library holds: gemm256p_kernel<bn, epilogue, f8, conv> (written out independently of gemm_main_instantiated)."""
    if conv:
        return not f8 and bn in (256, 128) and epi in (EPI_F32, EPI_BIAS_BF16, EPI_BIAS_RESID)
    if f8:
        return (bn in (256, 128) and epi in (EPI_F32, EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID)) or (bn == 192 and epi == EPI_BIAS_RESID)
    return epi in {384: (EPI_BIAS_BF16, EPI_BIAS_RESID), 192: (EPI_QKV_ATTN, EPI_BIAS_RESID),
                   256: (EPI_F32, EPI_QKV, EPI_QKV_LN, EPI_BIAS_BF16, EPI_BIAS_RESID, EPI_UP_DWCONV2, EPI_UP_DWCONV32),
                   128: (EPI_F32, EPI_QKV, EPI_QKV_LN, EPI_BIAS_BF16, EPI_BIAS_RESID)}.get(bn, ())


def test_invariants_over_the_sweep(sweep):
    for q, p in sweep:
        c = lambda n: q[:, Q[n]].astype(np.int64)
        M, N, K, epi, ncu = c("M"), c("N"), c("K"), c("epilogue"), c("ncu")
        f8, conv, ksplit = c("f8") != 0, c("conv") != 0, c("ksplit")
        fam, bn, bm, ring, nb = p[:, FAMILY], p[:, BN].astype(np.int64), p[:, BM], p[:, RING] != 0, p[:, NBLOCKS].astype(np.int64)
        main = fam == MAIN
        ntm, ntn = (M + 255) // 256, (N + np.maximum(bn, 1) - 1) // np.maximum(bn, 1)
        splitk = (epi == EPI_F32) & (ksplit > 1) & ~f8 & ~conv

        # the LayerNorm-1 partial sums are defined on 96-column wave tiles: the residual add at N % 192 == 0 never sees 128- / 256-wide tiles, whatever M and the CU count
        resid192 = (epi == EPI_BIAS_RESID) & ~f8 & ~conv & (N % 192 == 0)
        assert (np.isin(bn[resid192 & main], (192, 384))).all() and (np.isin(fam[resid192], (MAIN, DOWN_PP))).all()
        assert (bn[fam == DOWN_PP] == 192).all()
        # the 384-wide bias tile only for the K it was built and tested for
        assert (K[main & (bn == 384) & (epi == EPI_BIAS_BF16)] >= 384).all()
        # ring: only 256-wide, only a whole number of its two-K-tile iterations, never fp8 + conv or fp8 + residual add, never split-K
        whole = np.where(conv, (9 * (c("cv_cin") // 64)) % 2 == 0, np.where(f8, (K >= 256) & (K % 256 == 0), (K >= 128) & (K % 128 == 0)))
        assert (whole[ring] & (bn[ring] == 256) & main[ring]).all()
        assert not (ring & f8 & (conv | (epi == EPI_BIAS_RESID))).any() and not (ring & splitk).any()
        assert not (ring & f8 & (c("f8_ring") == 0)).any()
        # split-K: 128-wide on the two-stage loop, whichever kernel
        assert (bn[splitk & (fam != REFUSED)] == 128).all() and np.isin(fam[splitk], (MAIN, SPLITK_PP)).all()
        # XCD groups: an even number of tile columns, >= 8 tile rows, a full grid, CUs in eights
        x2 = p[:, XCD] == 2
        assert np.isin(p[:, XCD], (0, 2)).all() and (main[x2] & (ntn[x2] % 2 == 0) & (ntm[x2] >= 8) & (nb[x2] == ncu[x2]) & (ncu[x2] % 8 == 0)).all()
        assert np.isin(epi[x2], (EPI_UP_DWCONV2, EPI_UP_DWCONV32, EPI_BIAS_BF16)).all()
        # the small-batch forms: only for their epilogue, with their switch on, on shapes their kernels are written for, within their tiles-per-CU limit
        fits = (~f8 & ~conv & (c("w_batch_rows") == 0) & (M * c("lda") * 2 < 2 ** 32) & (N * c("ldw") * 2 < 2 ** 32) & (c("lda") * 2 < 2 ** 24) & (c("ldw") * 2 < 2 ** 24))
        updw_ok = fits & (M % 256 == 0) & (N % 128 == 0) & (K % 128 == 0) & (K >= 256) & (c("ldo") % 4 == 0)
        u, s, d = fam == UPDW_PP, fam == SPLITK_PP, fam == DOWN_PP
        assert ((epi[u] == EPI_UP_DWCONV2) & updw_ok[u] & (c("updw_small")[u] != 0) & (nb[u] == (M[u] // 256) * (N[u] // 128)) & (nb[u] <= ncu[u])).all()
        assert (splitk[s] & updw_ok[s] & (c("has_c_f32")[s] != 0) & (c("splitk_small")[s] != 0) & (nb[s] == (M[s] // 256) * (N[s] // 128) * ksplit[s]) & (nb[s] <= 2 * ncu[s])).all()
        down_ok = fits & (ksplit <= 1) & (M % 64 == 0) & (N % 192 == 0) & (K % 64 == 0) & (K >= 192) & (c("ldr") % 4 == 0) & (c("has_bias") != 0) & (c("has_resid") != 0)
        assert ((epi[d] == EPI_BIAS_RESID) & down_ok[d] & (c("down_small")[d] != 0) & np.isin(bm[d], (64, 128)) & (M[d] % bm[d] == 0) & (nb[d] == (M[d] // bm[d]) * (N[d] // 192))
                & (nb[d] <= ncu[d])).all()
        assert (bm[d & ((M // 64) * (N // 192) <= ncu)] == 64).all()
        # ... and they ARE taken whenever all of that holds (the kernels they stand in for give the same bits, so this is about speed only)
        assert u[(epi == EPI_UP_DWCONV2) & updw_ok & (c("updw_small") != 0) & ((M // 256) * (N // 128) <= ncu)].all()
        # grids: one persistent 8-wave workgroup per CU, fewer when there are fewer work items; 4-wave forms one (split-K: two) per CU
        items = ntm * ntn * np.where(splitk, ksplit, 1)
        assert (nb[main] == np.minimum(items, ncu)[main]).all() and (p[main, BLOCK] == 512).all() and (bm[main] == 256).all()
        assert (p[u | s | d, BLOCK] == 256).all() and (p[u | s | d][:, [RING, XCD, HALF_TAIL]] == 0).all()
        assert (p[main, HALF_TAIL] == c("half_tail")[main]).all()
        # no plan names a kernel that is not built
        keys = np.unique(np.stack([bn[main], epi[main], f8[main], conv[main]], axis=1), axis=0)
        assert all(_instantiated(int(b), int(e), bool(f), bool(cv)) for b, e, f, cv in keys), keys


def test_resid_stat_slots_follow_the_wave_tiles():
    """gemm_resid_stat_slots(N) = N / 96 relies on the residual-add invariant above: every width it accepts (N % 192 == 0, at most 8 slots) gets 192- / 384-wide tiles
    or the 4-wave form at every M -- the widths of the sweep that qualify are 192, 384, 768."""
    for N in (192, 384, 768):
        for ncu in (256, 304, 60):
            for M in MS:
                p = plan(M, N, 3072, EPI_BIAS_RESID, ncu=ncu)
                assert (p[FAMILY] == DOWN_PP and p[BN] == 192) or (p[FAMILY] == MAIN and p[BN] in (192, 384)), (M, N, ncu, p)


def test_plan_header_is_host_only():
    """csrc/tld_gemm_plan.h: plain C++ -- no HIP include, no environment, no state."""
    import os
    import re
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(here, "transformer_latent_diffusion_amd", "csrc")
    for name in ("tld_gemm_plan.h", "tld_gemm_params.h"):
        src = open(os.path.join(csrc, name)).read()
        assert re.findall(r"#include\s+[<\"]([^>\"]+)", src) == {"tld_gemm_plan.h": ["tld_gemm_params.h"], "tld_gemm_params.h": ["stdint.h"]}[name]
        assert "getenv" not in src and not re.search(r"\bstatic\b", src)
    # the five switches are read in exactly one function of the two GEMM translation units
    gemm = open(os.path.join(csrc, "tld_gemm.hip")).read() + open(os.path.join(csrc, "tld_updw.hip")).read()
    assert sorted(re.findall(r'on\("(TLD_\w+)"\)', gemm)) == ["TLD_DOWN_SMALL", "TLD_F8_RING", "TLD_GEMM_HALFTAIL", "TLD_SPLITK_SMALL", "TLD_UPDW_SMALL"]
    assert len(re.findall(r"getenv\(", gemm)) == 3          # gemm_switches()'s one call + the two of the TLD_DBG_EPI attribution build

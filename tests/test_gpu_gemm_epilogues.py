"""Every GEMM kernel class the plan can name, outside conv / the fused depthwise epilogues / fused attention, against the same operation in float64.

tld_debug_gemm_epilogue (include/tld_hip.h) runs ONE launch_gemm call on the test's own buffers.  CASES below is the whole list; the CPU test
test_cases_reach_every_kernel_class feeds it through plan_gemm and holds the set of (epilogue, f8, family, bn, bm, ring, xcd_ngroups, half-tail active)
it reaches against the frozen table tests/golden/g20_gemm_plans.npz (256 CUs, all switches on).  No class is unreachable through the entry point.

Per element, never through a norm.  The bound of one output element is derived, not tuned (see _acc_term and the epilogue references):
  a correct kernel accumulates the exact products of its operands in fp32 and rounds the result once to bf16 --
    |out - ref| <= 2^-8 |ref|                                  the rounding to bf16: 8 significant bits, so nearest is up to 2^-8 relative just above a power of two
                 + 2e-5 max|A W^T| sqrt(K / 64) + 1e-5         the fp32 accumulation bound test_gemm_bf16_vs_fp32_matmul asserts for the fp32 epilogue
                                                               (fp8: 5e-5 max|A W^T| sqrt(K / 128) + 1e-6, the one test_mx8_gemm_equals_product_of_dequantised_operands asserts)
                 + 2^-22 (sum of the magnitudes of the epilogue's fp32 terms)     its two or three fp32 additions / fmas, 2^-24 relative each
  LayerNorm folds, out = rstd_m (acc - mean_m c1[n]) + b[n]: the accumulation term is multiplied by rstd_m and |rstd_m mean_m c1[n]| joins the fp32 terms; where
  the kernel derives (mean, rstd) itself from fp32 partial sums (EPI_QKV_LN), var = E[x^2] - mean^2 loses 2^-23 E[x^2] / var relative, half of which reaches rstd.
Measured maxima of error / bound per case: profiles/r08_gemm_epilogue_errors.txt.

What these tests found: gemm256p_kernel<384, EPI_BIAS_BF16> had no epilogue at all (the if-constexpr chain went from the residual add to WCOLS == 64) and stored
nothing -- every 32768 x 768 linear of the training step at batch 128, and the VAE shape tld_gemm_plan.h records as 'came out wrong in every row'."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_gemm_plan import ALL_ON, BM, BN, FAMILY, HALF_TAIL, NBLOCKS, Q, RING, XCD, plan, sweep_chunk

EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID, EPI_QKV_LN = 1, 2, 3, 5
EPI_NAME = {1: "QKV", 2: "BIAS_BF16", 3: "BIAS_RESID", 5: "QKV_LN"}
NCU = 256                     # the CU count the coverage below is computed for (MI355X)
PATTERN = 0x7FA5              # guard-band fill: a bf16 NaN no kernel produces
LN_EPS = 1e-5                 # kLnEps (csrc/tld_common.h)

# (epilogue, operand mode, M, N, K, extras).  extras: ntok (QKV: tokens per sample; d = N / 3), ln3 (EPI_BIAS_BF16 with row_stats + ln_c1), stats (EPI_BIAS_RESID
# with stats_out), pad (ldo / ldr = N + pad, q | k: 2 d + pad)
CASES = [
    # ---- EPI_BIAS_BF16, bf16 operands
    (EPI_BIAS_BF16, "bf16", 32768, 768, 384, {}),                  # the training step's linears at batch 128: 256 x 384 tiles, two XCD column groups
    (EPI_BIAS_BF16, "bf16", 32768, 768, 768, {"pad": 8}),
    (EPI_BIAS_BF16, "bf16", 32768, 768, 3072, {}),
    (EPI_BIAS_BF16, "bf16", 65536, 384, 384, {}),                  # 384-wide, one tile column (no XCD groups)
    (EPI_BIAS_BF16, "bf16", 65536, 384, 128, {}),                  # the VAE shape that 'came out wrong in every row' on the 384-wide tile; 128-wide since
    (EPI_BIAS_BF16, "bf16", 4928, 768, 768, {}),                   # CLIP: 64 prompts x 77 tokens
    (EPI_BIAS_BF16, "bf16", 4928, 2304, 768, {}),
    (EPI_BIAS_BF16, "bf16", 4928, 3072, 768, {"ln3": 1}),
    (EPI_BIAS_BF16, "bf16", 300, 200, 64, {"ln3": 1, "pad": 8}),   # ragged M and N, the smallest K
    (EPI_BIAS_BF16, "bf16", 1000, 1000, 128, {"ln3": 1}),
    (EPI_BIAS_BF16, "bf16", 1000, 200, 192, {}),
    (EPI_BIAS_BF16, "bf16", 1000, 1000, 320, {"pad": 24}),
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 64, {}),                   # 256-wide, two-stage loop, XCD groups, ragged M
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 192, {"ln3": 1}),
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 320, {}),
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 128, {}),                  # ... on the ring
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 256, {"ln3": 1}),
    (EPI_BIAS_BF16, "bf16", 8152, 2048, 384, {"pad": 8}),
    (EPI_BIAS_BF16, "bf16", 12200, 2048, 256, {"ln3": 1}),
    (EPI_BIAS_BF16, "bf16", 2048, 4608, 192, {}),                  # 128-wide with XCD groups
    (EPI_BIAS_BF16, "bf16", 3584, 4608, 192, {}),                  # 256-wide without them, two-stage loop
    (EPI_BIAS_BF16, "bf16", 3584, 4608, 128, {"ln3": 1}),          # ... ring
    (EPI_BIAS_BF16, "bf16", 8192, 2304, 256, {"ln3": 1}),          # ring with the half-tile tail
    (EPI_BIAS_BF16, "bf16", 8192, 2304, 128, {}),
    # ---- EPI_QKV / EPI_QKV_LN, bf16 operands
    (EPI_QKV, "bf16", 16384, 2304, 768, {"ntok": 1024}),           # the denoiser's QKV at C3: 256-wide, ring, half-tile tail
    (EPI_QKV_LN, "bf16", 16384, 2304, 768, {"ntok": 1024}),
    (EPI_QKV, "bf16", 16448, 2304, 768, {"ntok": 64}),             # 257 samples of 64 tokens: the last one ends in a ragged tile
    (EPI_QKV_LN, "bf16", 16448, 2304, 768, {"ntok": 64, "pad": 8}),
    (EPI_QKV, "bf16", 832, 576, 192, {"ntok": 64}),                # d = 192: 13 samples, 3.25 tile rows
    (EPI_QKV_LN, "bf16", 832, 576, 192, {"ntok": 64}),
    (EPI_QKV, "bf16", 1280, 1152, 384, {"ntok": 256, "pad": 16}),  # d = 384
    (EPI_QKV_LN, "bf16", 1280, 1152, 384, {"ntok": 256}),
    (EPI_QKV, "bf16", 4928, 2304, 768, {"ntok": 616}),             # 4928 rows as 8 samples of 616 tokens: samples straddle tiles
    (EPI_QKV_LN, "bf16", 1000, 576, 64, {"ntok": 200}),
    (EPI_QKV, "bf16", 3584, 4608, 192, {"ntok": 256}),             # 256-wide on the two-stage loop
    (EPI_QKV_LN, "bf16", 3584, 4608, 320, {"ntok": 256}),
    (EPI_QKV, "bf16", 3584, 4608, 128, {"ntok": 256}),             # ring, whole rounds
    (EPI_QKV_LN, "bf16", 3584, 4608, 256, {"ntok": 256}),
    (EPI_QKV, "bf16", 4096, 4608, 128, {"ntok": 1024}),            # ring with the half-tile tail at the smallest K it takes
    (EPI_QKV_LN, "bf16", 4096, 4608, 384, {"ntok": 1024}),
    # ---- EPI_BIAS_RESID, bf16 operands
    (EPI_BIAS_RESID, "bf16", 32768, 768, 64, {"stats": 1}),        # the 384-wide tile at K < 384: no test reached these
    (EPI_BIAS_RESID, "bf16", 32768, 768, 128, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 32768, 768, 192, {"stats": 1, "pad": 4}),
    (EPI_BIAS_RESID, "bf16", 32768, 768, 256, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 32768, 768, 320, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 32768, 768, 3072, {"stats": 1}),      # the down projection at the bench size
    (EPI_BIAS_RESID, "bf16", 65536, 384, 64, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 65536, 384, 128, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 65536, 384, 192, {}),
    (EPI_BIAS_RESID, "bf16", 65536, 384, 256, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 65536, 384, 320, {"stats": 1}),       # the largest case
    (EPI_BIAS_RESID, "bf16", 8152, 3072, 64, {}),                  # 384-wide, ragged M, N = 3072: no slots
    (EPI_BIAS_RESID, "bf16", 4928, 768, 3072, {"stats": 1}),       # CLIP's down projection: 192-wide
    (EPI_BIAS_RESID, "bf16", 1000, 192, 192, {"stats": 1, "pad": 4}),
    (EPI_BIAS_RESID, "bf16", 300, 384, 64, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 12200, 384, 128, {"stats": 1}),
    (EPI_BIAS_RESID, "bf16", 8152, 768, 384, {"stats": 1, "pad": 12}),
    (EPI_BIAS_RESID, "bf16", 1000, 3072, 256, {}),                 # 192-wide, stats_out null
    (EPI_BIAS_RESID, "bf16", 64, 192, 192, {"stats": 1}),          # the 4-wave form, 64-row tiles
    (EPI_BIAS_RESID, "bf16", 512, 768, 3072, {"stats": 1}),        # ... one image at C1
    (EPI_BIAS_RESID, "bf16", 1536, 2304, 192, {}),                 # ... 128-row tiles
    (EPI_BIAS_RESID, "bf16", 300, 200, 64, {"pad": 4}),            # 128-wide, ragged both ways
    (EPI_BIAS_RESID, "bf16", 1000, 1000, 320, {}),
    (EPI_BIAS_RESID, "bf16", 14336, 1024, 192, {}),                # 256-wide, two-stage loop
    (EPI_BIAS_RESID, "bf16", 14336, 1024, 128, {"pad": 8}),        # ... ring
    # ---- MX-fp8 operands (quantised by tld_debug_quant_mx8, bit-exact in test_gpu_fp8.py)
    (EPI_QKV, "fp8", 832, 576, 128, {"ntok": 64}),                 # 128-wide
    (EPI_QKV, "fp8", 1024, 768, 128, {"ntok": 256}),               # 256-wide, two-stage loop
    (EPI_QKV, "fp8", 1280, 768, 256, {"ntok": 64}),                # ring, ragged last tile
    (EPI_QKV, "fp8", 4096, 4608, 256, {"ntok": 1024}),             # ring with the half-tile tail
    (EPI_BIAS_BF16, "fp8", 1000, 200, 128, {"pad": 8}),
    (EPI_BIAS_BF16, "fp8", 32768, 192, 128, {}),                   # 128-wide with XCD groups
    (EPI_BIAS_BF16, "fp8", 1000, 256, 384, {}),
    (EPI_BIAS_BF16, "fp8", 4096, 4608, 128, {}),                   # 256-wide with XCD groups
    (EPI_BIAS_BF16, "fp8", 1000, 256, 256, {}),                    # ring
    (EPI_BIAS_BF16, "fp8", 8192, 2304, 256, {}),                   # ring with the half-tile tail
    (EPI_BIAS_BF16, "fp8", 4096, 4608, 256, {}),                   # ring with XCD groups
    (EPI_BIAS_RESID, "fp8", 1000, 200, 128, {"pad": 4}),
    (EPI_BIAS_RESID, "fp8", 1000, 192, 128, {}),                   # 192-wide
    (EPI_BIAS_RESID, "fp8", 32768, 768, 384, {}),
    (EPI_BIAS_RESID, "fp8", 65536, 768, 256, {}),                  # the down projection at C4: 256-wide
    (EPI_BIAS_RESID, "fp8", 1000, 256, 128, {}),
]


def case_id(c):
    epi, mode, M, N, K, ex = c
    return f"{EPI_NAME[epi]}-{mode}-{M}x{N}x{K}" + "".join(f"-{k}{v}" for k, v in ex.items())


def case_plan(c, M=None, switches=ALL_ON):
    epi, mode, cm, N, K, ex = c
    M = cm if M is None else M
    pad = ex.get("pad", 0)
    ldo = (2 * (N // 3) if epi in (EPI_QKV, EPI_QKV_LN) else N) + pad
    return plan(M, N, K, epi, ncu=NCU, switches=switches, f8=1 if mode == "fp8" else 0, ldo=ldo, ldr=N + pad)


def half_tail_active(M, N, epi, p):
    """gemm256p_kernel's own condition (tld_gemm.hip): HT_OK (ring, no conv, an epilogue that can skip one row half), the launch's half_tail, no XCD groups, and
    on some XCD a last round of R left-over tiles for P workgroups with 0 < 2 R <= P."""
    if p[FAMILY] != 1 or not p[RING] or not p[HALF_TAIL] or p[XCD] > 1 or epi not in (0, EPI_QKV, EPI_QKV_LN, EPI_BIAS_BF16):
        return 0
    bn, nblocks = int(p[BN]), int(p[NBLOCKS])
    ntiles = ((M + 255) // 256) * ((N + bn - 1) // bn)
    for xcd in range(8):
        per_xcd_blocks = (nblocks + 7 - xcd) // 8
        if per_xcd_blocks == 0:
            continue
        xcount = (ntiles >> 3) + (1 if xcd < (ntiles & 7) else 0)
        ht_R = xcount - (xcount // per_xcd_blocks) * per_xcd_blocks
        if ht_R > 0 and 2 * ht_R <= per_xcd_blocks:
            return 1
    return 0


def kernel_class(epi, f8, M, N, p):
    return (int(epi), int(f8), int(p[FAMILY]), int(p[BN]), int(p[BM]), int(p[RING]), int(p[XCD]), half_tail_active(M, N, epi, p))


def describe(p):
    return (f"plan(family {p[FAMILY]}, tile {p[BM]} x {p[BN]}, ring {p[RING]}, xcd_ngroups {p[XCD]}, half_tail {p[HALF_TAIL]}, {p[NBLOCKS]} workgroups)")


# ---- coverage, on the CPU ------------------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_kernel_class():
    """Every class of the frozen table (256 CUs, all switches on) with one of the four epilogues and conv == 0 is reached by a case; printed: class -> first case."""
    g = load_golden("g20_gemm_plans.npz")
    assert tuple(g["variants"][0]) == (NCU,) + ALL_ON
    q = sweep_chunk(NCU, ALL_ON)
    plans = g["distinct_plans"][g["plan_index"][g["offsets"][0]:g["offsets"][1]]]
    keep = np.isin(q[:, Q["epilogue"]], (EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID, EPI_QKV_LN)) & (q[:, Q["conv"]] == 0) & (plans[:, FAMILY] != 0)
    table = {kernel_class(r[Q["epilogue"]], r[Q["f8"]], int(r[Q["M"]]), int(r[Q["N"]]), p) for r, p in zip(q[keep], plans[keep])}
    reached = {}
    for c in CASES:
        epi, mode, M, N, K, ex = c
        p = case_plan(c)
        assert p[FAMILY] != 0, (case_id(c), "refused")
        reached.setdefault(kernel_class(epi, mode == "fp8", M, N, p), case_id(c))
    for k in sorted(reached):
        print(k, "<-", reached[k])
    missing = sorted(table - set(reached))
    assert not missing, f"classes (epilogue, f8, family, bn, bm, ring, xcd_ngroups, half-tail active) of the frozen table that no case reaches: {missing}"
    assert len(table) == 38          # 26 (epilogue, operands, family, tile, K loop) classes, split further by XCD groups and an active half-tile tail
    assert len({case_id(c) for c in CASES}) == len(CASES)


def test_cases_are_what_the_entry_point_accepts():
    """The shapes respect what tld_debug_gemm_epilogue validates, so a refusal on the GPU is a finding and not a typo here."""
    for c in CASES:
        epi, mode, M, N, K, ex = c
        assert K % (128 if mode == "fp8" else 64) == 0 and (mode != "fp8" or (M % 4 == 0 and N % 4 == 0)), case_id(c)
        assert ex.get("pad", 0) % (4 if epi == EPI_BIAS_RESID else 8) == 0
        if epi in (EPI_QKV, EPI_QKV_LN):
            assert N % 3 == 0 and (N // 3) % 64 == 0 and ex["ntok"] % 8 == 0 and M % ex["ntok"] == 0, case_id(c)
            assert epi == EPI_QKV or (mode == "bf16" and _ln_slots(K) <= 8), case_id(c)
        elif epi == EPI_BIAS_BF16:
            assert N % 8 == 0 and (not ex.get("ln3") or (M % 2 == 0 and mode == "bf16" and not (N % 384 == 0 and N < 1536))), case_id(c)
        else:
            assert N % 4 == 0 and (not ex.get("stats") or (mode == "bf16" and N % 192 == 0 and N // 96 <= 8)), case_id(c)


# ---- the launch and its float64 reference ---------------------------------------------------------------------------------------------------------------------
def _ln_slots(K):
    n = -(-K // 96)
    return n + (n & 1)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded(rows, ld, guard_rows, dev):
    """bf16 [rows + guard_rows][ld], every element the guard pattern."""
    return torch.full((rows + guard_rows, ld), PATTERN, dtype=torch.int16, device=dev).view(torch.bfloat16)


def _e4m3_lut(dev):
    return torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().double().to(dev)


def make_inputs(c, dev):
    """Operands and side inputs of a case, from a device generator seeded by the shape (the child process of the half-tail check rebuilds the same bits)."""
    from transformer_latent_diffusion_amd import _lib
    epi, mode, M, N, K, ex = c
    g = torch.Generator(device=dev).manual_seed(1000003 * epi + 7919 * M + 31 * N + K + (1 if mode == "fp8" else 0))
    rn = lambda *s: torch.randn(*s, generator=g, device=dev)
    I = {}
    folded = epi == EPI_QKV_LN or ex.get("ln3")
    if mode == "fp8":
        a = rn(M, K) * torch.exp(rn(M, K // 32) * 1.5).repeat_interleave(32, 1)
        w = rn(N, K) * 0.1 * torch.exp(rn(N, K // 32)).repeat_interleave(32, 1)
    elif folded:
        a = rn(M, K) * torch.exp(rn(M, 1) * 0.7) + rn(M, 1) * 0.5          # the raw residual stream: a mean and a scale per row
        w = rn(N, K) * 0.1 * (1 + 0.3 * rn(1, K))                          # gamma-scaled weights
    else:
        a, w = rn(M, K), rn(N, K) * 0.1
    a, w = a.to(torch.bfloat16).contiguous(), w.to(torch.bfloat16).contiguous()
    if mode == "fp8":
        lut = _e4m3_lut(dev)
        for name, x, rows in (("A", a, M), ("W", w, N)):
            qx = torch.empty(rows, K, dtype=torch.uint8, device=dev)
            sc = torch.zeros(K // 128, rows, 4, dtype=torch.uint8, device=dev)
            _lib.check(_lib.lib().tld_debug_quant_mx8(x.data_ptr(), qx.data_ptr(), sc.data_ptr(), rows, K, _stream()), "quant_mx8")
            torch.cuda.synchronize()
            e8 = sc.permute(1, 0, 2).reshape(rows, K // 32)                # [K/128][rows][4] -> [rows][K/32]
            I[name], I[name + "_scale"] = qx, sc
            I[name + "64"] = (lut[qx.long()].view(rows, K // 32, 32) * torch.pow(2.0, e8.double() - 127)[..., None]).view(rows, K)
    else:
        I["A"], I["W"], I["A64"], I["W64"] = a, w, a.double(), w.double()
    I["bias"] = (rn(N) * 0.5 + torch.arange(N, device=dev) * 1e-3).float().contiguous()         # differs per column
    if epi == EPI_BIAS_RESID:
        I["resid0"] = (rn(M, N) * 2 + torch.arange(M, device=dev)[:, None] * 1e-4).to(torch.bfloat16)      # differs per row and column
    if folded:
        I["c1"] = I["W64"].sum(1).float().contiguous()
    if ex.get("ln3"):
        x = I["A64"]
        mean = x.mean(1)
        I["row_stats"] = torch.stack([mean, 1.0 / torch.sqrt(x.var(1, unbiased=False) + LN_EPS)], 1).float().contiguous()
    if epi == EPI_QKV_LN:
        slots = _ln_slots(K)
        xp = torch.zeros(M, 8 * 96, dtype=torch.float64, device=dev)
        xp[:, :K] = I["A64"]
        xp = xp.view(M, 8, 96)
        st = torch.stack([xp.sum(2), (xp * xp).sum(2)], 2).float()          # [M][8] (sum, sum of squares), one slot per 96 columns
        st[:, slots:] = 1e30                                                # slots past ln_slots are not the kernel's to read
        I["ln_stats"], I["ln_slots"] = st.contiguous(), slots
    return I


def launch(c, I, dev, row_ranges=None):
    """Runs the case (as one launch, or one launch per row range) into fresh guarded buffers; returns them."""
    from transformer_latent_diffusion_amd import _lib
    epi, mode, M, N, K, ex = c
    pad = ex.get("pad", 0)
    O = {}
    if epi == EPI_BIAS_RESID:
        O["ld"] = N + pad
        O["resid"] = _guarded(M, O["ld"], 256, dev)
        O["resid"][:M, :N] = I["resid0"]
        if ex.get("stats"):
            O["stats"] = torch.full((M + 256, 8, 2), 0x7FA5A5A5, dtype=torch.int32, device=dev).view(torch.float32)
    elif epi == EPI_BIAS_BF16:
        O["ld"] = N + pad
        O["out"] = _guarded(M, O["ld"], 256, dev)
    else:
        d, ntok = N // 3, ex["ntok"]
        O["ld"] = 2 * d + pad
        O["out"] = _guarded(M, O["ld"], 256, dev)
        O["vt"] = _guarded((M // ntok + -(-256 // ntok)) * d, ntok, 0, dev)         # [B + guard samples][d][ntok]
    esz = 1 if mode == "fp8" else 2
    for r0, r1 in (row_ranges or [(0, M)]):
        a = _lib.TldGemmEpilogueArgs()
        a.A, a.W = I["A"].data_ptr() + r0 * K * esz, I["W"].data_ptr()
        a.M, a.N, a.K, a.lda, a.ldw, a.epilogue, a.f8 = r1 - r0, N, K, K, K, epi, 1 if mode == "fp8" else 0
        if mode == "fp8":
            # [K/128][M][4]: a row range of the scales is not contiguous -- gather it
            sc = I["A_scale"][:, r0:r1].contiguous()
            O.setdefault("keep", []).append(sc)
            a.a_scale, a.w_scale = sc.data_ptr(), I["W_scale"].data_ptr()
        a.bias = I["bias"].data_ptr() if epi in (EPI_BIAS_BF16, EPI_BIAS_RESID) else None
        if epi == EPI_BIAS_RESID:
            a.resid, a.ldr = O["resid"].data_ptr() + r0 * O["ld"] * 2, O["ld"]
            if "stats" in O:
                a.stats_out = O["stats"].data_ptr() + r0 * 64
        else:
            a.out_bf16, a.ldo = O["out"].data_ptr() + r0 * O["ld"] * 2, O["ld"]
        if ex.get("ln3"):
            a.row_stats, a.ln_c1 = I["row_stats"].data_ptr() + r0 * 8, I["c1"].data_ptr()
        if epi in (EPI_QKV, EPI_QKV_LN):
            a.ntok, a.d = ex["ntok"], N // 3
            a.vt = O["vt"].data_ptr() + (r0 // ex["ntok"]) * (N // 3) * ex["ntok"] * 2
        if epi == EPI_QKV_LN:
            a.ln_stats, a.ln_slots, a.ln_c1, a.ln_b1 = I["ln_stats"].data_ptr() + r0 * 64, I["ln_slots"], I["c1"].data_ptr(), I["bias"].data_ptr()
        _lib.check(_lib.lib().tld_debug_gemm_epilogue(C.byref(a), _stream()), f"tld_debug_gemm_epilogue({case_id(c)}, rows {r0}:{r1})")
    torch.cuda.synchronize()
    return O


def _acc_term(c, prod):
    """The fp32 accumulation bound of the existing fp32-epilogue tests (docstring above), from the float64 product's own scale."""
    K, scale = c[4], prod.abs().max().item()
    return 5e-5 * scale * np.sqrt(K / 128) + 1e-6 if c[1] == "fp8" else 2e-5 * scale * np.sqrt(K / 64) + 1e-5


def reference(c, I):
    """(ref, bound), float64 [M][N]: what the epilogue stores, before its rounding to bf16, and the bound of one element."""
    epi, mode, M, N, K, ex = c
    prod = I["A64"] @ I["W64"].t()
    acc = _acc_term(c, prod)
    u = 2.0 ** -22
    if epi == EPI_QKV:
        ref, bound = prod, acc + torch.zeros_like(prod)
    elif epi == EPI_BIAS_RESID:
        b, r0 = I["bias"].double()[None, :], I["resid0"].double()
        ref = r0 + (prod + b)
        bound = acc + u * (prod.abs() + b.abs() + r0.abs())
    elif epi == EPI_BIAS_BF16 and not ex.get("ln3"):
        b = I["bias"].double()[None, :]
        ref = prod + b
        bound = acc + u * (prod.abs() + b.abs())
    else:
        # out = rstd_m (acc - mean_m c1[n]) + b[n]
        b, c1 = I["bias"].double()[None, :], I["c1"].double()[None, :]
        if epi == EPI_QKV_LN:
            st = I["ln_stats"].double()[:, :I["ln_slots"]]
            mean, ex2 = st[:, :, 0].sum(1) / K, st[:, :, 1].sum(1) / K
            var = (ex2 - mean * mean).clamp(min=0)
            rstd = 1.0 / torch.sqrt(var + LN_EPS)
            # the kernel forms var in fp32: 2^-23 E[x^2] absolute, half of it relative to (var + eps) in rstd; + the hardware rsq (1 ulp) and the partial-sum adds
            rstd_rel = 2.0 ** -23 * (ex2 / (var + LN_EPS) + 8)
        else:
            mean, rstd = I["row_stats"].double()[:, 0], I["row_stats"].double()[:, 1]
            rstd_rel = torch.zeros_like(mean)
        mean, rstd, rstd_rel = mean[:, None], rstd[:, None], rstd_rel[:, None]
        ref = rstd * (prod - mean * c1) + b
        bound = rstd * acc + u * (rstd * prod.abs() + (rstd * mean * c1).abs() + b.abs()) + rstd_rel * (rstd * prod.abs() + 2 * (rstd * mean * c1).abs())
    return ref, bound + 2.0 ** -8 * ref.abs()


def _first_bad(bad, bm, bn):
    i = int(torch.nonzero(bad.reshape(-1))[0])
    r, cidx = divmod(i, bad.shape[1])
    return r, cidx, f"tile ({r // bm}, {cidx // bn})"


def check_values(c, p, what, got, ref, bound, col0=0):
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                      # (NaN and the guard pattern count as bad)
    ratio = float((err / bound).nan_to_num(nan=float("inf")).max())
    print(f"{case_id(c)} {what}: max error / bound {ratio:.3f}")
    if bad.any():
        r, cc, tile = _first_bad(bad, int(p[BM]), int(p[BN]))
        raise AssertionError(f"{case_id(c)} {what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; first at (row {r}, column {col0 + cc}), {tile} of the launch: "
                             f"got {float(got[r, cc])}, reference {float(ref[r, cc])}, bound {float(bound[r, cc]):.3e}; {describe(p)}")
    return ratio


def check_guard(c, p, what, buf, rows, cols):
    """Everything of the [rows + guard][ld] buffer outside [:rows, :cols] still holds the fill pattern."""
    raw = buf.view(torch.int16)
    touched = raw != torch.tensor(PATTERN, dtype=torch.int16, device=raw.device)
    touched[:rows, :cols] = False
    if touched.any():
        r, cc, tile = _first_bad(touched, int(p[BM]), int(p[BN]))
        raise AssertionError(f"{case_id(c)} {what}: {int(touched.sum())} guard elements overwritten; first at (row {r}, column {cc}) of a [{rows}][{cols}] region "
                             f"with pitch {raw.shape[1]}, {tile}; {describe(p)}")


def check_case(c, I, O, p):
    """All per-element checks of one launch's outputs; returns the largest error / bound."""
    epi, mode, M, N, K, ex = c
    ref, bound = reference(c, I)
    worst = 0.0
    if epi == EPI_BIAS_RESID:
        check_guard(c, p, "residual", O["resid"], M, N)
        worst = check_values(c, p, "residual", O["resid"][:M, :N], ref, bound)
        if "stats" in O:
            nslot = N // 96
            raw = O["stats"].view(torch.int32)
            untouched = raw == 0x7FA5A5A5
            assert untouched[M:].all() and untouched[:M, nslot:].all(), f"{case_id(c)}: stats_out written past row {M} or past slot {nslot}; {describe(p)}"
            # sums OF THE STORED VALUES: 96 fp32 additions (fmas) per slot, 2^-24 relative each on a running sum of at most sum |x| (sum x^2)
            x = O["resid"][:M, :N].double().view(M, nslot, 96)
            for j, (want, mag) in enumerate(((x.sum(2), x.abs().sum(2)), ((x * x).sum(2), (x * x).sum(2)))):
                r = check_values(c, p, ("stats_out sums", "stats_out sums of squares")[j], O["stats"][:M, :nslot, j], want, 97 * 2.0 ** -24 * mag + 1e-30)
                worst = max(worst, r)
    elif epi == EPI_BIAS_BF16:
        check_guard(c, p, "output", O["out"], M, N)
        worst = check_values(c, p, "output", O["out"][:M, :N], ref, bound)
    else:
        d, ntok = N // 3, ex["ntok"]
        B = M // ntok
        check_guard(c, p, "q | k", O["out"], M, 2 * d)
        worst = check_values(c, p, "q | k", O["out"][:M, :2 * d], ref[:, :2 * d], bound[:, :2 * d])
        check_guard(c, p, "V^T", O["vt"], B * d, ntok)
        vt = O["vt"][:B * d].view(B, d, ntok).permute(0, 2, 1).reshape(M, d)          # back to [row][feature]: (row, column) of the launch
        to_rows = lambda t: t[:, 2 * d:].contiguous()
        worst = max(worst, check_values(c, p, "V^T", vt, to_rows(ref), to_rows(bound), col0=2 * d))
    return worst


def outputs_equal(c, p, O1, O2, how):
    for k in ("resid", "out", "vt", "stats"):
        if k in O1:
            a, b = O1[k].view(torch.int16 if k != "stats" else torch.int32), O2[k].view(torch.int16 if k != "stats" else torch.int32)
            if not torch.equal(a, b):
                a2, b2 = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
                r, cc, _ = _first_bad(a2 != b2, 1, 1)
                raise AssertionError(f"{case_id(c)}: {k} differs bitwise {how}: {int((a2 != b2).sum())} elements, first at (row {r}, column {cc}); {describe(p)}")


def split_ranges(c):
    """Two launches of half the rows each, where half the rows are still a shape the entry point accepts; None otherwise."""
    epi, mode, M, N, K, ex = c
    h = M // 2
    unit = ex["ntok"] if epi in (EPI_QKV, EPI_QKV_LN) else (4 if mode == "fp8" else 2)
    h -= h % unit
    return [(0, h), (h, M)] if 0 < h < M else None


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_epilogue_against_float64(c, tmp_path):
    dev = torch.device("cuda:0")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    if ncu != NCU:
        pytest.skip(f"the kernel-class coverage of these cases is computed for {NCU} CUs; this device has {ncu}")
    epi, mode, M, N, K, ex = c
    p = case_plan(c)
    I = make_inputs(c, dev)
    O = launch(c, I, dev)
    check_case(c, I, O, p)
    # independence of the cut (tld_gemm_plan.h: 'results do not depend on the tile width', 'must not depend on the batch size'): the same rows as two launches
    rr = split_ranges(c)
    if rr is not None:
        outputs_equal(c, p, O, launch(c, I, dev, rr), f"between one launch and two launches of rows {rr} ({describe(case_plan(c, rr[0][1]))} / {describe(case_plan(c, M - rr[0][1]))})")
    # ... and, where the half-tile tail is active, without it (the switch is read once per process: a fresh child)
    if half_tail_active(M, N, epi, p):
        path = str(tmp_path / "halftail_off.pt")
        tests = os.path.dirname(os.path.abspath(__file__))
        code = (f"import sys; sys.path.insert(0, {tests!r}); sys.path.insert(0, {os.path.dirname(tests)!r})\n"
                "import torch, test_gpu_gemm_epilogues as t\n"
                f"c = t.CASES[{CASES.index(c)}]; dev = torch.device('cuda:0')\n"
                "O = t.launch(c, t.make_inputs(c, dev), dev)\n"
                f"torch.save({{k: v.cpu() for k, v in O.items() if k in ('resid', 'out', 'vt', 'stats')}}, {path!r})\n")
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, TLD_GEMM_HALFTAIL="0"), capture_output=True, text=True, cwd=os.path.dirname(tests), timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        O0 = {k: v.to(dev) for k, v in torch.load(path).items()}
        outputs_equal(c, p, {k: O[k] for k in O0}, O0, "between the run with the half-tile tail and TLD_GEMM_HALFTAIL=0")


def test_entry_point_refuses_what_the_kernels_assume():
    """CPU: every refusal comes before the first HIP call, names the entry point in tld_last_error and launches nothing (the pointers are host memory)."""
    from transformer_latent_diffusion_amd import _lib
    mem = np.zeros(1 << 12, np.uint8)
    ptr = (mem.ctypes.data + 63) & ~63
    base = dict(A=ptr, W=ptr, bias=ptr, out_bf16=ptr, resid=ptr, vt=ptr, M=64, N=192, K=64, lda=64, ldw=64, ldo=192, ldr=192, epilogue=EPI_BIAS_BF16)
    ln = dict(epilogue=EPI_QKV_LN, ldo=128, ntok=64, d=64, ln_stats=ptr, ln_c1=ptr, ln_b1=ptr)
    bads = [dict(epilogue=4), dict(epilogue=6), dict(epilogue=7), dict(epilogue=8), dict(K=96, lda=96, ldw=96), dict(K=0), dict(lda=32), dict(N=196), dict(bias=None),
            dict(out_bf16=None), dict(ldo=196), dict(ldo=184), dict(A=ptr + 2), dict(bias=ptr + 4),
            dict(epilogue=0), dict(epilogue=0, c_f32=ptr, ldc=100),
            dict(epilogue=EPI_BIAS_RESID, resid=None), dict(epilogue=EPI_BIAS_RESID, ldr=194), dict(epilogue=EPI_BIAS_RESID, N=190), dict(epilogue=EPI_BIAS_RESID, ldr=188),
            dict(epilogue=EPI_BIAS_RESID, N=256, ldr=256, stats_out=ptr), dict(epilogue=EPI_BIAS_RESID, N=960, ldr=960, stats_out=ptr),
            dict(epilogue=EPI_BIAS_RESID, f8=1, K=128, lda=128, ldw=128, a_scale=ptr, w_scale=ptr, stats_out=ptr),
            dict(epilogue=EPI_QKV, ldo=128, ntok=64, d=48), dict(epilogue=EPI_QKV, ldo=128, ntok=60, d=64), dict(epilogue=EPI_QKV, ldo=128, ntok=48, d=64),
            dict(epilogue=EPI_QKV, ldo=120, ntok=64, d=64), dict(epilogue=EPI_QKV, ldo=128, ntok=64, d=64, vt=None), dict(epilogue=EPI_QKV, ldo=128, ntok=64, d=128),
            dict(ln, ln_slots=3), dict(ln, ln_slots=10), dict(ln, ln_slots=0), dict(ln, ln_slots=2, ln_stats=None), dict(ln, ln_slots=2, f8=1, K=128, lda=128, ldw=128, a_scale=ptr, w_scale=ptr),
            dict(row_stats=ptr), dict(row_stats=ptr, ln_c1=ptr, N=768, ldo=768), dict(row_stats=ptr, ln_c1=ptr, M=62 + 1),
            dict(row_stats=ptr, ln_c1=ptr, f8=1, K=128, lda=128, ldw=128, a_scale=ptr, w_scale=ptr),
            dict(f8=1, K=128, lda=128, ldw=128), dict(f8=1, K=64, a_scale=ptr, w_scale=ptr), dict(f8=1, K=128, lda=128, ldw=128, a_scale=ptr, w_scale=ptr, M=62),
            dict(w_batch_rows=128, M=256), dict(epilogue=EPI_BIAS_RESID, w_batch_rows=256, M=512)]
    for bad in bads:
        a = _lib.TldGemmEpilogueArgs()
        for k, v in {**base, **bad}.items():
            setattr(a, k, v)
        assert _lib.lib().tld_debug_gemm_epilogue(C.byref(a), None) == 1, bad
        assert b"tld_debug_gemm_epilogue" in _lib.lib().tld_last_error(), bad
    assert _lib.lib().tld_debug_gemm_epilogue(None, None) == 1
    assert not mem.any()

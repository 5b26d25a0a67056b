// tld_gemm_plan.h -- which kernel a launch_gemm call gets: ONE pure function of the launch's shape, the CU count and five switches.
//
// Host-only integer arithmetic (no HIP, no environment, no state), so the whole selection can be tabulated and tested without a GPU:
// tld_debug_gemm_plan (include/tld_hip.h) exposes it, tests/test_gemm_plan.py holds it against a frozen table, named shapes and the
// invariants written beside the clauses below.  launch_gemm (tld_gemm.hip) only executes the plan.
#pragma once
#include "tld_gemm_params.h"

#ifndef TLD_KLOOP_RING
#define TLD_KLOOP_RING 1      // counted-vmcnt half-tile ring K loop for 256 x 256 tiles (see kloop_ring); 0 = never instantiate it (the two-stage staggered loop everywhere)
#endif

namespace tld {

enum GemmFamily {
    GEMM_REFUSED = 0,        // nothing is launched; GemmPlan::refusal says why
    GEMM_MAIN = 1,           // gemm256p_kernel<bn, epilogue, f8, conv, ring>: 8 waves, 256-row tiles, one persistent workgroup per CU (tld_gemm.hip)
    GEMM_UPDW_PP = 2,        // updw_pp_kernel<0>: EPI_UP_DWCONV2 on 256 x 128 tiles, 4 waves (tld_updw.hip)
    GEMM_SPLITK_PP = 3,      // updw_pp_kernel<1>: EPI_F32 split-K slices on the same K loop
    GEMM_DOWN_PP = 4,        // down_pp_kernel<bm / 64>: EPI_BIAS_RESID on 64 x 192 or 128 x 192 tiles, 4 waves
};
enum GemmRefusal { GEMM_OK = 0, GEMM_REFUSED_CONV_UP_DOWN = 1, GEMM_REFUSED_NO_KERNEL = 2 };

inline const char* gemm_refusal_text(int refusal) {
    switch (refusal) {
        case GEMM_REFUSED_CONV_UP_DOWN: return "launch_gemm: conv with both cv_up and cv_down set";
        case GEMM_REFUSED_NO_KERNEL: return "launch_gemm: no kernel is built for this combination of epilogue, operand mode (bf16 / fp8 / conv) and tile width";
        default: return "";
    }
}

struct GemmPlan {
    int family;              // GemmFamily
    int bn, bm;              // tile: bn columns (main: 128 / 192 / 256 / 384) x bm rows
    int ring;                // main: the half-tile ring K loop (else the two-stage loop)
    int xcd_ngroups;         // GemmParams::xcd_ngroups of the launch (2 or 0)
    int half_tail;           // GemmParams::half_tail of the launch (main: the switch; the kernel applies it on the ring, see HT_OK)
    int nblocks, block;      // grid and workgroup size
    int refusal;             // GemmRefusal
};

// A/B and test hooks, all on by default; 0 in the environment variable of the same name (TLD_...) turns one off.  Read once per process by gemm_switches() (tld_gemm.hip).
struct GemmSwitches {
    bool f8_ring = true;         // TLD_F8_RING=0: the two-stage loop under the fp8 GEMMs (rounds 2 - 5)
    bool half_tail = true;       // TLD_GEMM_HALFTAIL=0: no row-split tail (tests/test_gpu_parity.py holds it bitwise equal to the unsplit run)
    bool updw_small = true;      // TLD_UPDW_SMALL=0, TLD_SPLITK_SMALL=0, TLD_DOWN_SMALL=0: the 8-wave kernels at small batch as well (bitwise the same results)
    bool splitk_small = true;
    bool down_small = true;
};

// The chip the thresholds below were measured on (MI355X: 8 XCDs x 32 CUs).  Tile WIDTH is chosen against these constants, not against the CU count of
// the device (grids, XCD groups and the small-batch limits do use it).  ADVICE item 5 -- derive them from the CU count, skip the half-tail clause of
// bf16_tile_width when the tail is off -- changes which kernel runs and is a change to these three lines with a visible diff of the frozen table.
constexpr long kPlanCus = 256, kPlanXcds = 8, kPlanCusPerXcd = 32;

// ---- what is built ---------------------------------------------------------------------------------------------------------------------------------------
// The instantiations of gemm256p_kernel<bn, epilogue, f8, conv> in the library; launch_gemm's dispatch has one case per combination accepted here.
constexpr bool gemm_main_instantiated(int bn, int epilogue, bool f8, bool conv) {
    const bool plain = epilogue == EPI_F32 || epilogue == EPI_BIAS_BF16 || epilogue == EPI_BIAS_RESID;
    if (conv) return !f8 && plain && (bn == 256 || bn == 128);             // implicit 3x3 convolution (VAE): three epilogues
    if (f8) return (bn == 256 || bn == 128) ? (plain || epilogue == EPI_QKV) : (bn == 192 && epilogue == EPI_BIAS_RESID);      // MX-fp8: four epilogues, 192-wide for the residual add
    switch (bn) {
        case 384: return epilogue == EPI_BIAS_BF16 || epilogue == EPI_BIAS_RESID || epilogue == EPI_QKV_ATTN2;       // two heads of QKV + attention; residual add (the down projection) and, for the training step's N = 768 linears, bias -> bf16
        case 192: return epilogue == EPI_QKV_ATTN || epilogue == EPI_BIAS_RESID;
        case 256: return plain || epilogue == EPI_QKV || epilogue == EPI_QKV_LN || epilogue == EPI_UP_DWCONV2 || epilogue == EPI_UP_DWCONV32;
        case 128: return plain || epilogue == EPI_QKV || epilogue == EPI_QKV_LN;
        default: return false;
    }
}
// ... and those that also exist on the ring K loop: 256 x 256 tiles
// (fp8 + residual-add epilogue on the ring: 172 spilled registers, also with the lane-derived values re-materialised -- that one stays on the two-stage loop)
constexpr bool gemm_ring_instantiated(int bn, int epilogue, bool f8, bool conv) {
    return TLD_KLOOP_RING && bn == 256 && !(f8 && (conv || epilogue == EPI_BIAS_RESID)) && gemm_main_instantiated(bn, epilogue, f8, conv);
}

// ---- the reach of the tile DMA ---------------------------------------------------------------------------------------------------------------------------------
// The DMA of a plain (non-conv, non-TN) launch forms each operand row's address as a uniform 64-bit base plus a 32-bit
// byte offset  row * pitch (__umul24: both factors < 2^24)  + the 16-byte piece inside the row's first 128 bytes (+ the
// block-diagonal group's W offset).  The largest such offset must not wrap: (M - 1) lda ESZ + 128 <= 2^32 for A, and
// (N - 1) ldw ESZ + 128 + the last group's offset for W.  Host arithmetic only: launch_gemm asks it before every launch, and the engines' create
// (tld_reach.h) keep every launch of theirs inside it.
constexpr const char* kGemmReachRefusal =
    "launch_gemm: an operand row lies beyond the 4 GiB reach of the 32-bit DMA offsets (row * pitch + 128 bytes must stay "
    "<= 2^32 for A and for W); split the launch by rows";
inline int gemm_offsets_fit(const GemmParams& p) {
    const uint64_t esz = p.f8 ? 1 : 2, lim = 1ull << 32;
    const uint64_t pa = (uint64_t)p.lda * esz, pw = (uint64_t)p.ldw * esz;
    if (p.M < 1 || p.N < 1 || p.M > (1 << 24) || p.N > (1 << 24) || pa >= (1u << 24) || pw >= (1u << 24)) return 0;
    if ((uint64_t)(p.M - 1) * pa + 128 > lim) return 0;
    const uint64_t wgrp = p.w_batch_rows ? (uint64_t)((p.M - 1) / p.w_batch_rows) * p.w_batch_stride_bytes : 0;
    return (uint64_t)(p.N - 1) * pw + 128 + wgrp <= lim;
}

// ---- the 4-wave small-batch forms (tld_updw.hip): shapes their kernels are written for ------------------------------------------------------------------------
// (all three: bf16 operands whose byte offsets fit the kernels' 32-bit DMA offsets and 24-bit multiplies)
inline bool pp_operands_fit(const GemmParams& p) {
    return !p.f8 && !p.conv && !p.w_batch_rows && (uint64_t)p.M * p.lda * 2 < ((uint64_t)1 << 32) && (uint64_t)p.N * p.ldw * 2 < ((uint64_t)1 << 32) &&
           (unsigned)p.lda * 2u < (1u << 24) && (unsigned)p.ldw * 2u < (1u << 24);
}
// EPI_UP_DWCONV2 on 256 x 128 tiles: bitwise equal to the 8-wave kernel
inline bool updw_pp_supported(const GemmParams& p) {
    return pp_operands_fit(p) && p.M % 256 == 0 && p.N % 128 == 0 && p.K % 128 == 0 && p.K >= 256 && p.ldo % 4 == 0;
}
// EPI_F32 with ksplit > 1 on the same K loop: K = the length of ONE split (a multiple of 128, >= 256); bitwise the slices of gemm256p_kernel<128, EPI_F32>
inline bool splitk_pp_supported(const GemmParams& p) {
    return p.ksplit > 1 && p.c_f32 != nullptr && updw_pp_supported(p);
}
// EPI_BIAS_RESID of the default class on 64 x 192 or 128 x 192 tiles: bitwise gemm256p_kernel<192 | 384, EPI_BIAS_RESID>
inline bool down_pp_supported(const GemmParams& p) {
    return pp_operands_fit(p) && p.ksplit <= 1 && p.M % 64 == 0 && p.N % 192 == 0 && p.K % 64 == 0 && p.K >= 192 && p.ldr % 4 == 0 && p.bias && p.resid;
}

// ---- tile width of the 8-wave kernel, bf16 operands, no conv, no split-K -------------------------------------------------------------------------------------------
// Results do not depend on the tile width (every output element sees the same K order), so the choice may follow the batch size -- with ONE exception, the
// residual-add epilogue at N % 192 == 0, see below.
inline int bf16_tile_width(long M, long N, long K, int epilogue) {
    const long ntm = (M + 255) / 256;
    auto whole_rounds = [&](long bn) { return N % bn == 0 && (ntm * (N / bn)) % kPlanCus == 0; };       // the workgroups of bn-wide tiles fill every round of the chip
    if (epilogue == EPI_QKV_ATTN) return 192;          // one tile = one (sample, head): caller guarantees N = heads x 192, ntok == 256
    if (epilogue == EPI_QKV_ATTN2) return 384;         // one tile = one (sample, head pair): the caller asked plan_qkv_pair first
    if (epilogue == EPI_UP_DWCONV2 || epilogue == EPI_UP_DWCONV32) return 256;          // caller guarantees N % 256 == 0 and one 16x16 image (8 rows of a 32x32 one) per 256 rows
    // INVARIANT (gemm_resid_stat_slots below relies on it): the residual-add epilogue at N % 192 == 0 uses 192- or 384-wide tiles for EVERY batch size, never
    // 128 / 256 -- both give 96-column wave tiles, which is what the LayerNorm-1 partial sums are defined on (results must not depend on the batch size).
    // 384-wide where that makes whole rounds: the down projection at the bench size, N = 768, is ONE round of 256 workgroups (176 -> 155 us).
    if (epilogue == EPI_BIAS_RESID && N % 192 == 0) return whole_rounds(384) ? 384 : 192;
    // N = 768 with the plain bias epilogue (the training step's five per layer): one round of 256 x 384 tiles at the training batch instead of three rounds of
    // 256 x 128 (0.71 -> 1.0 PFLOP/s).  N < 1536: callers with a LayerNorm-3 fold have N = 4 d >= 1536, and the 384-wide tile has no room for the fold.
    // K >= 384: the shapes it was built for.  The VAE's attention projection at 128 channels and 65 536 tokens -- N = 384, K = 128, 256 tile-rows --
    // met the other conditions and came out wrong in every row; it takes the 128-wide tiles like every other K = 128 launch.
    // The cause had nothing to do with K: gemm256p_kernel<384, EPI_BIAS_BF16> had no epilogue.  Its wave tiles are 96 columns wide, the bias -> bf16 store code was
    // written under `WCOLS == 64`, and the if-constexpr chain of epilogues simply ended -- the kernel ran its K loop and stored nothing, at every K (the VAE saw it
    // because its output buffer is read; the training step at batch 128, the shape this tile was built for, has no test at that size).  The 96-column epilogue exists
    // now and tests/test_gpu_gemm_epilogues.py holds the tile against float64 at K = 384, 768 and 3072; the clause stays because those are the K it is tested at
    // (and the frozen table records it).  The same tile under the residual add has no such clause and needs none: its epilogue handles 96-column wave tiles, and
    // the same tests hold it at K = 64 .. 320.
    if (epilogue == EPI_BIAS_BF16 && N < 1536 && K >= 384 && whole_rounds(384)) return 384;
    // Everything else: 256 unless the width does not divide, or that leaves the last round of workgroups mostly empty; then 128.
    // (a last round that is at least 85 % full counts as whole: 252 tiles on 256 CUs are not a reason to halve the tile)
    const long blocks256 = ntm * ((N + 255) / 256), rounds256 = (blocks256 + kPlanCus - 1) / kPlanCus;
    if (N % 256 != 0) return 128;
    if (!(blocks256 * 100 < rounds256 * kPlanCus * 85 && blocks256 < 3 * kPlanCus)) return 256;
    // Round 6: a partly filled last round is cheap where the half-tile tail applies (gemm256p_kernel, HT_OK epilogues on the ring K loop): when the R left-over
    // tiles of an XCD's 32 workgroups satisfy 2 R <= 32, two workgroups share each of them and the launch costs q + ~0.6 tile times instead of q + 1.  256-wide
    // tiles then beat twice as many 128-wide ones (C3's block-0 QKV projection, 16 384 rows x 2304: 576 tiles = 2.25 rounds; 84 us as 1152 tiles of 128).
    // (Does not look at GemmSwitches::half_tail or xcd_ngroups: ADVICE item 5.)
    const bool tail_epilogue = epilogue == EPI_F32 || epilogue == EPI_QKV || epilogue == EPI_QKV_LN || epilogue == EPI_BIAS_BF16;
    if (tail_epilogue && K >= 128 && K % 128 == 0 && blocks256 >= kPlanCus && blocks256 % kPlanXcds == 0) {
        const long R = (blocks256 / kPlanXcds) % kPlanCusPerXcd;
        if (R > 0 && 2 * R <= kPlanCusPerXcd) return 256;
    }
    return 128;
}

// Slots of LayerNorm-1 partial sums an EPI_BIAS_RESID launch of width N writes for every batch size (0: shape not supported -> keep the LN kernel).  One slot per
// 96-column wave tile: the invariant of bf16_tile_width, which the 4-wave form (192-wide tiles, the same wave tiles) keeps.
inline int gemm_resid_stat_slots(int N) {
    return (N % 192 == 0 && N / 96 <= kLnSlots) ? N / 96 : 0;
}

// ---- the plan -----------------------------------------------------------------------------------------------------------------------------------------------------
inline GemmPlan plan_gemm(const GemmParams& p, int epilogue, int ncu, const GemmSwitches& sw) {
    auto refused = [](int why) { return GemmPlan{GEMM_REFUSED, 0, 0, 0, 0, 0, 0, 0, why}; };
    auto small = [](int family, int bm, int bn, long nblocks) { return GemmPlan{family, bn, bm, 0, 0, 0, (int)nblocks, 256, GEMM_OK}; };
    const bool f8 = p.f8 != 0, conv = p.conv != 0;
    const bool splitk = epilogue == EPI_F32 && p.ksplit > 1 && !f8 && !conv;        // (ksplit is ignored by every other epilogue and operand mode)

    // 1. Refusals that need no further look.
    if (conv && p.cv_up && p.cv_down) return refused(GEMM_REFUSED_CONV_UP_DOWN);    // upsampling and stride 2 are exclusive addressing modes
    if (conv && f8) return refused(GEMM_REFUSED_NO_KERNEL);

    // 2. Small batches: 4-wave workgroups with one tile each while the launch leaves the chip mostly empty.  Each form is bitwise equal to the 8-wave kernel it stands
    //    in for (tests/test_gpu_dwconv.py, test_gpu_low_latency.py), so the choice may follow the batch size.
    if (epilogue == EPI_UP_DWCONV2 && sw.updw_small && updw_pp_supported(p)) {
        // one to five images per call: one 256 x 128 tile per workgroup on twice as many CUs finishes sooner than one 256 x 256 tile (17.7 vs 28.6 us at one image).
        // At most ONE tile per CU: two such workgroups fit a CU, but this epilogue does not share it well -- 288 - 480 tiles on two workgroups per CU measured
        // 1 - 2 ms per generate slower than the 8-wave kernel.
        const long tiles = (long)(p.M / 256) * (p.N / 128);
        if (tiles <= ncu) return small(GEMM_UPDW_PP, 256, 128, tiles);
    }
    if (splitk && sw.splitk_small && splitk_pp_supported(p)) {
        // the low-latency classes' split-K down projection: one 256 x 128 x (K / splits) item per workgroup while the launch has at most TWO items per CU
        // (K loops only share a CU well: eight images in class 1 -- 384 items -- 58.3 -> 48.8 ms per generate)
        const long items = (long)(p.M / 256) * (p.N / 128) * p.ksplit;
        if (items <= 2L * ncu) return small(GEMM_SPLITK_PP, 256, 128, items);
    }
    if (epilogue == EPI_BIAS_RESID && !f8 && !conv && sw.down_small && down_pp_supported(p)) {
        // the default class's down projection: at most one tile per CU, 64-row tiles while they fit, else 128-row ones
        const long n64 = (long)(p.M / 64) * (p.N / 192), n128 = (long)(p.M / 128) * (p.N / 192);
        if (n64 <= ncu) return small(GEMM_DOWN_PP, 64, 192, n64);
        if (p.M % 128 == 0 && n128 <= ncu) return small(GEMM_DOWN_PP, 128, 192, n128);
    }

    // 3. The 8-wave kernel: tile width by operand mode.
    const long ntm = ((long)p.M + 255) / 256;
    auto whole_rounds = [&](long w) { return p.N % w == 0 && (ntm * (p.N / w)) % kPlanCus == 0; };
    int bn;
    if (conv) {
        bn = (p.N % 256 == 0 && 4 * ntm * (p.N / 256) >= 3 * kPlanCus) ? 256 : 128;      // 256-wide tiles when the width allows and they fill (three quarters of) the chip
    } else if (f8) {
        // 256 / 128 for all four epilogues and 192 for the residual add (N = 768 in whole rounds).  Round 6: where 256-wide tiles fill whole rounds they beat the
        // 192-wide ones -- the down projection at C4, 65 536 rows: 768 tiles in 3 rounds against 1024 in 4, 207.7 -> 174.8 us same-box (the LayerNorm-1 partial
        // sums are not taken in fp8 mode, so the invariant of bf16_tile_width does not bind here)
        if (epilogue == EPI_BIAS_RESID && whole_rounds(256)) bn = 256;
        else if (epilogue == EPI_BIAS_RESID && p.N % 192 == 0 && (whole_rounds(192) || p.N % 256 != 0)) bn = 192;
        else bn = p.N % 256 == 0 ? 256 : 128;
    } else if (splitk) {
        bn = 128;           // the narrow tile has no ring instantiation to fall into (split-K runs on the two-stage loop) and gives the most work items
    } else {
        bn = bf16_tile_width(p.M, p.N, p.K, epilogue);
    }
    // (A column-split QKV launch -- 8 tile-columns of 256 as 4 whole rounds + the 9th as 128-wide tiles -- was measured: 109.8 + 27.8 us vs 134 us for the single
    // 4.5-round launch; a one-round launch pays ~12 us of ramp/drain, so the half-empty fifth round is the cheaper tail.)
    if (!gemm_main_instantiated(bn, epilogue, f8, conv)) return refused(GEMM_REFUSED_NO_KERNEL);

    // 4. K loop: the half-tile ring where it is built and K is a whole number of its iterations -- two 128-byte K-tiles: 128 bf16 or 256 fp8 elements; conv: the
    //    9 cv_cin / 64 K-tiles of all taps together.
    const bool whole_ring_iterations = conv ? (9 * (p.cv_cin >> 6)) % 2 == 0 : f8 ? (p.K >= 256 && p.K % 256 == 0) : (p.K >= 128 && p.K % 128 == 0);
    const bool ring = gemm_ring_instantiated(bn, epilogue, f8, conv) && whole_ring_iterations && (!f8 || sw.f8_ring);

    // 5. Grid: one persistent workgroup per CU, fewer when there are fewer tiles.
    const long ntn = ((long)p.N + bn - 1) / bn, tiles = ntm * ntn * (splitk ? p.ksplit : 1);
    const long nblocks = tiles < ncu ? tiles : ncu;

    // 6. XCD groups.  Up-projection (12 tile-columns at d = 768): two column groups x four tile-row blocks over the 8 XCDs keep each XCD's W working set at 2.4 MB
    //    (L2-resident across rounds; it was re-fetched every round, PMC fetch 296 MB vs 55 MB algorithmic) while A is fetched by two XCDs instead of one: 235 -> 228 us.
    //    Measured and rejected: four groups for the up-projection (neutral), two / four groups for the down-projection (A is the 201 MB operand there: neutral /
    //    175 -> 195 us), two or four head groups for EPI_QKV_ATTN (round 4: PMC traffic 2.6 x algorithmic, but the kernel stayed at 131.7 us: not fetch-bound).
    //    Large launches only: every XCD cell needs workgroups of its own.
    const bool up_projection = epilogue == EPI_UP_DWCONV2 || epilogue == EPI_UP_DWCONV32 || epilogue == EPI_BIAS_BF16;
    const int xcd_ngroups = (up_projection && ntn % 2 == 0 && ntm >= 8 && nblocks == ncu && ncu % 8 == 0) ? 2 : 0;

    return GemmPlan{GEMM_MAIN, bn, 256, ring ? 1 : 0, xcd_ngroups, sw.half_tail ? 1 : 0, (int)nblocks, 512, GEMM_OK};
}

}  // namespace tld

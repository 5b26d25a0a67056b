// tld_gemm_params.h -- the GEMM launch descriptor (the kernel argument) and its epilogue constants, free of HIP so that host-only code
// (tld_gemm_plan.h: which kernel a launch gets) can read them.  Device code sees them through tld_common.h.
#pragma once
#include <stdint.h>
#ifndef __HIP__
struct float2;      // HIP's vector type, which a plain C++ translation unit only meets behind GemmParams' pointers
#endif

namespace tld {

#if defined(__clang__) || (defined(__GNUC__) && __GNUC__ >= 13)
typedef __bf16 bf16;
#else
struct __bf16 { uint16_t bits; };      // a host compiler without the type (tests/host/body_plan_main.cpp) only meets it behind pointers and in sizeof
typedef __bf16 bf16;
#endif

// Residual stream dtype: bf16, as in the reference's own bf16 mode (x never leaves bf16 there either).  All
// statistics, softmax and residual ADDS are computed in fp32 and rounded once on store.  Measured vs the fp32
// reference: forward rel-rms 5-7e-3, 35-step CFG-6 trajectory 1.4e-2 (tolerances 2e-2 / 6e-2; the reference's
// own bf16 path is at 0.8-1.0e-2 per forward).  -DTLD_RESID_FP32 keeps x in fp32 (2.7e-3 / 4.6e-3, ~4 % slower).
#ifdef TLD_RESID_FP32
typedef float resid_t;
#else
#define TLD_RESID_BF16 1
typedef __bf16 resid_t;
#endif

constexpr int kLnSlots = 8;      // LayerNorm-1 partial-sum slots per row (one per 96-column group; see GemmParams::stats_out)

enum GemmEpilogue {
    EPI_F32 = 0,         // C fp32 [M,N]                         (debug / small tables)
    EPI_QKV = 1,         // q,k -> bf16 [M,2d] ; v -> bf16 transposed per (sample, head): [B,H,64,Ntok]
    EPI_BIAS_BF16 = 2,   // bf16(C + bias[n]) -> [M,N]           (MLP up projection)
    EPI_BIAS_RESID = 3,  // x[m,n] += C + bias[n] (resid_t)      (MLP down projection)
    EPI_QKV_LN = 5,      // EPI_QKV with LayerNorm-1 folded in (A = raw residual stream, see GemmParams::ln_stats)
    EPI_UP_DWCONV32 = 4, // the same on a 32 x 32 token grid (a tile = 8 image rows): interior rows here, seam rows by launch_dwconv_seam (round 4; a separate
                         //   instantiation so that the 16 x 16 kernel's register allocation stays what it was)
    EPI_UP_DWCONV2 = 6,  // bf16(C + bias) -> depthwise 3x3 + bias + GELU over the tile's 16x16 image -> [M,N]  (MLP up projection fused with
                         // the depthwise conv: token-pair image in LDS, packed-bf16 taps on v_dot2c_f32_bf16; needs ntok == 256, BN == 256.
                         // Value 4 was the first form of this epilogue, retired in round 4.)
    EPI_QKV_ATTN = 7,    // QKV GEMM (LayerNorm-1 folded in) + the head's whole self-attention in the epilogue: W rows are permuted to
                         // [head][q_h | k_h | v_h] so that a 256 x 192 tile = everything (sample, head) needs; q, k, v go from the
                         // accumulators to LDS, softmax(q k^T / 8) v runs there, and only att[256 x 64] is written (out_bf16, ldo = d).
                         // Needs ntok == 256, N = 3 d = heads x 192, K % 128 == 0.  (tld/transformer_blocks.py:51-59 + 24-48)
    EPI_QKV_ATTN2 = 9,   // the same on 256 x 384 tiles, TWO heads per tile: W rows in pair order (tld_refresh_math.h: qkv_pair_row), the second head's
                         // k and v in LDS images of their own and its q parked in GemmParams::park while the first head's attention runs.  Bitwise the results of EPI_QKV_ATTN.  Heads even.
                         // (8 is not used: kernel names with template argument 8 are read as an up-projection form by the benchmark's trace reader)
};

struct GemmParams {
    const bf16* A; int lda;       // [M,K] row-major, K contiguous
    const bf16* W; int ldw;       // [N,K] row-major (nn.Linear weight layout)
    int M, N, K;
    float* c_f32; int ldc;        // EPI_F32
    bf16* out_bf16; int ldo;      // EPI_QKV (q|k, ldo = 2d) / EPI_BIAS_BF16
    bf16* vt;                     // EPI_QKV
    int ntok, d;                  // EPI_QKV
    const float* bias;            // EPI_BIAS_*
    const float* dw_b;            // EPI_UP_DWCONV2: HALVED depthwise bias [N]  (the epilogue's GELU takes x / 2)
    uint32_t* dw_seam;            // EPI_UP_DWCONV32: the epilogue computes the six interior rows of its 8 image rows (+ the image's own top / bottom row) and leaves
                                  //   rows 0, 1, 6, 7 of the hidden tensor, in its token-pair image format, here for launch_dwconv_seam:
                                  //   [M / 256 tiles][N / 256 column tiles][64 pair-rows][256 channels] dwords
    const uint32_t* dw_wpk;       // EPI_UP_DWCONV2: HALVED depthwise taps as packed bf16 pairs [3 window rows][4 kinds][N]:
                                  //   kinds (lo, hi): (0, w0), (w1, w2) for even output columns; (w0, w1), (w2, 0) for odd ones
    resid_t* resid; int ldr;      // EPI_BIAS_RESID
    // LayerNorm-1 folded into the QKV GEMM (EPI_QKV_LN): the producers of the residual stream (embed, EPI_BIAS_RESID)
    // leave per-row partial sums (sum x, sum x^2) of the ROUNDED values, one slot per 96-column group (slot index =
    // column / 96, the same for 192- and 384-wide tiles, so results do not depend on the tile shape chosen for a
    // batch size); the QKV GEMM multiplies the raw residual by bf16(gamma1 (.) Wqkv) and its epilogue applies
    // rstd_m (acc - mean_m c1[n]) + b1[n].
    float2* stats_out;            // EPI_BIAS_RESID: [M][kLnSlots] partials out (null: none)
    const float2* ln_stats;       // EPI_QKV_LN: [M][kLnSlots] partials of the A rows
    int ln_slots;                 // EPI_QKV_LN: slots to sum per row (even, <= kLnSlots)
    const float* ln_b1;           // EPI_QKV_LN: [N] beta1 . Wqkv^T   (ln_c1 below holds the column sums)
    // EPI_UP_DWCONV2 / EPI_BIAS_BF16 with LayerNorm-3 folded in: A is the raw bf16 residual stream, W = bf16(gamma3 (.) Wup),
    // bias = up_b + beta3 . Wup^T, and the image write applies  rstd_m (acc - mean_m c1[n]) + bias[n]
    const float2* row_stats;      // [M] (mean, rstd) per row; null: A is already normalized
    const float* ln_c1;           // [N] column sums of the gamma-scaled bf16 weights
    // MX-fp8 operands (f8 != 0): A and W hold OCP e4m3 bytes ([M,K] / [N,K], K contiguous, lda / ldw in elements = bytes),
    // a_scale / w_scale one E8M0 byte per 32 K-elements, laid out [K/128][rows][4] so that a tile's scales of one 128-wide
    // K-step are contiguous.  K % 128 == 0, M % 4 == 0, N % 4 == 0.  Epilogues: EPI_F32, EPI_QKV, EPI_BIAS_BF16, EPI_BIAS_RESID.
    int f8;
    const uint8_t* a_scale;
    const uint8_t* w_scale;
    // Implicit 3x3 convolution (conv != 0; VAE decoder, tld_vae.hip): the A operand is never materialised.  Row m of the GEMM is
    // output pixel (b, y, x) of a channels-last [B, cv_h, cv_w, *] image, K = 9 cv_cin with k = tap * cv_cin + c (tap = 3 ky + kx,
    // W laid out [N][3][3][cv_cin]), and K-step k of a tile is DMA'd from the 128-byte channel slice of source pixel
    // (y + ky - 1, x + kx - 1) -- or of ((y + ky - 1) >> 1, (x + kx - 1) >> 1) in a half-resolution source when cv_up (nearest
    // 2x upsampling folded into the addressing).  A points at the activation BUFFER, whose first cv_data_off bytes are
    // zeros (>= 2 cv_cin: one whole pixel): taps outside the image read that zero pixel, so there is no border code in
    // the kernel.
    // cv_cin % 64 == 0; buffer size < 4 GiB; epilogues EPI_F32, EPI_BIAS_BF16, EPI_BIAS_RESID; 256- and 128-wide tiles.
    // Block-diagonal batching of the W operand (w_batch_rows != 0; EPI_F32 / EPI_BIAS_BF16 only): the A rows are w_batch_rows-row
    // groups stacked into one tall matrix, and group g multiplies ITS OWN W matrix at byte offset g * w_batch_stride_bytes from W
    // (attention inside the VAE decoder: scores_b = Q_b K_b^T and O_b = P_b V_b for all samples in one launch each).
    // w_batch_rows % 256 == 0 (a tile never straddles groups); the offset stays inside the 32-bit DMA offsets.
    int w_batch_rows;
    unsigned w_batch_stride_bytes;
    int conv, cv_h, cv_w, cv_up, cv_cin;
    unsigned cv_data_off;
    // conv epilogues EPI_BIAS_BF16 / EPI_BIAS_RESID: GroupNorm statistics of the OUTPUT for its consumer, fused into the epilogue
    // (null: none).  partial[(sample, 256-pixel chunk)][group] = (sum, sum of squares) of the output values (bias-to-bf16 epilogue: before their rounding), gn_cpg channels per
    // group, gn_hw pixels per sample.  Requires gn_hw % 256 == 0 (a tile never straddles samples), N % 128 == 0, gn_cpg % 4 == 0.
    float2* gn_partial;
    int gn_groups, gn_cpg, gn_hw;
    int ksplit;                   // > 1 (EPI_F32, bf16, no conv): split-K -- K is the length of ONE split, split s multiplies columns [s K, (s + 1) K) of A and W (lda / ldw
                                  //   = the full row pitch) and writes its fp32 product to c_f32 + s M ldc; the caller sums the slices in a fixed order
    int xcd_ngroups;              // > 1: XCDs form a (8 / G) x G grid over (tile-rows, tile-column groups); needs ntn % G == 0
    // Transposed-operand form (launch_gemm_tn; the weight gradients dW = dY^T X of the training step): A [k rows][lda] and W [k rows][ldw] are
    // both row-major with the CONTRACTION index as the row, C[M, N] = sum_k A[k][m] W[k][n].  tn_ktotal = rows of both operands; K = rows per
    // split (multiple of 64); w_batch_rows != 0: output rows [j w_batch_rows, (j + 1) w_batch_rows) are split j = operand rows [j K, min((j + 1) K,
    // tn_ktotal)) against the same A columns (split-K into fp32 slices, summed by the caller in a fixed order).
    int tn_ktotal;
    int half_tail;                // ring K loop: split the tiles of a partly filled last round by ROWS between two workgroups (set by the launcher)
    int dbg_epi;                  // experiment knob, builds with -DTLD_DBG_EPI only (TLD_EPI_DBG bit mask, see tld_gemm.hip)
    int cv_down;                  // conv: stride-2 3x3 convolution with padding (0, 1, 0, 1) (diffusers Downsample2D, VAE encoder): output pixel (y, x)
                                  //   and tap (ky, kx) read source pixel (2y + ky, 2x + kx) of a 2 cv_h x 2 cv_w image -- a tap is outside only on the
                                  //   bottom / right pad, which reads the zero page.  Excludes cv_up (launch_gemm refuses both).
    uint32_t* park;               // EPI_QKV_ATTN2: one slot of kPairSlotDwords per workgroup of the launch (min(tiles, CUs) slots)
};

constexpr int kPairSlotDwords = 512 * 16;     // EPI_QKV_ATTN2: 512 lanes x 16 packed bf16 pairs = the second head's q of one 256 x 384 tile (32 KB); its k and v stay in LDS

}  // namespace tld

// tld_reach.h -- the sizes at which 32-bit (and 16-bit) arithmetic inside the kernels ends, as refusals: the table of DESIGN.md section 7.19 written as host
// code.  Most kernels form addresses in 64 bits; the few that do not -- the GEMM tile DMA (a 32-bit byte offset per lane), the row-streaming depthwise
// kernel (32-bit byte offsets and scale indices), the folded tail (32-bit element offsets) and every launch that puts samples or row chunks on a grid's y or
// z axis (65 535 blocks) -- rely on a bound that tld_engine_create, tld_train_create, the CLIP towers' create and the raw-buffer test hooks enforce HERE,
// before any allocation or launch.  A pure function of the sizes.  No HIP in this file: tests/host/reach_main.cpp compiles it on its own
// (tests/test_large_offsets_host.py), and tests/test_body_plan_host.py reaches the inference rules through tld_body_plan.h.
#pragma once

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../include/tld_hip.h"
#include "tld_gemm_plan.h"            // gemm_offsets_fit
#include "tld_launch_plan.h"          // plan_dwconv, plan_attention: the form and the workgroup count of the two hooks' launches
#include "tld_train_plan.h"           // kTrainTransposeMargin, train_dw_fused: the training step's workspace and forms

namespace tld {

constexpr uint64_t kReach32 = 1ull << 32;      // bytes (or elements) a 32-bit offset reaches
constexpr int64_t kGridYZ = 65535;             // blocks on the y or the z axis of a grid
constexpr int64_t kGridX = 2147483647;         // blocks on the x axis; also the largest int a launch's workgroup count is computed in

inline std::string reach_say(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline std::string reach_say(const char* fmt, ...) {
    char b[640];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}

// A buffer of per_sample x max_batch + extra bytes that is addressed through 32-bit offsets must stay below 4 GiB.  "" when it does; else the refusal, which
// names the buffer, how its size is formed and the largest max_batch that fits.
inline std::string reach_refusal(int max_batch, const char* buffer, const char* formula, uint64_t per_sample, uint64_t extra = 0) {
    const uint64_t bytes = per_sample * (uint64_t)max_batch + extra;
    if (bytes < kReach32) return std::string();
    const long long fits = extra < kReach32 ? (long long)((kReach32 - 1 - extra) / per_sample) : 0;
    return reach_say("max_batch=%d: %s (%s = %llu bytes) must stay below 4 GiB, the reach of the 32-bit offsets it is addressed through; the largest max_batch "
                     "that fits is %lld; run larger batches as several calls", max_batch, buffer, formula, (unsigned long long)bytes, fits);
}
// A launch that puts per_sample x max_batch blocks on a grid's y or z axis
inline std::string grid_refusal(int max_batch, const char* what, int64_t per_sample, int64_t limit = kGridYZ) {
    if (per_sample * (int64_t)max_batch <= limit) return std::string();
    return reach_say("max_batch=%d: %s (at most %lld); the largest max_batch that fits is %lld; run larger batches as several calls", max_batch, what, (long long)limit,
                     (long long)(limit / per_sample));
}

// ---- the inference engine (tld_engine_create, behind the hidden-activation rule of body_config_check) ---------------------------------------------------------
// `grid`: tokens per side.  The hidden activation [M, hid] bf16 is the A operand of the down projection (GEMM DMA), the output of the row-streaming depthwise
// kernel and an operand of the folded tail: its rule stands in body_config_check with the text it always had.  With mlp_multiplier >= 2 it is the largest
// activation buffer.  With mlp_multiplier 1 q|k [M, 2 d] bf16 is twice as large: its own kernels address it in 64 bits, but M <= 2^24 -- the row factor of the
// GEMM DMA's 24-bit multiply, which launch_gemm would otherwise refuse in the middle of a forward -- follows from it (2 d x 2 >= 256 bytes per row), and no
// activation buffer of 4 GiB or more has ever been executed.  In fp8 mode the e4m3 operand a8 [M, hid] is half the hidden activation, its scales as8 a 64th,
// and the seam buffer (32 x 32 tokens) [M hid / 4] dwords equals a8: none of them binds before the hidden activation does.
inline std::string body_reach_check(const tld_config& c, int grid) {
    const uint64_t ntok = (uint64_t)grid * grid;
    if (std::string bad = reach_refusal(c.max_batch, "the q|k activation", "max_batch x tokens x 2 embed_dim x 2 B", ntok * 2 * c.embed_dim * 2); !bad.empty()) return bad;
    return grid_refusal(c.max_batch, "the self-attention kernels put one sample on each block of the grid's z axis", 1);
}

// Every launch_gemm call of a forward of `batch` samples (run_body, tld_engine.hip) as (rows, row pitch in bytes) of its A operand; W operands are weights
// (at most 4 d rows of 4 d elements: 32 MiB).  What tests/host/reach_main.cpp asserts gemm_offsets_fit for at the largest accepted max_batch.
struct BodyGemm { const char* name; int M, N, K, lda; bool f8; };
inline int body_gemms(const tld_config& c, int grid, int batch, bool fp8, BodyGemm out[3]) {
    const int M = batch * grid * grid, d = c.embed_dim, hid = c.mlp_multiplier * c.embed_dim;
    out[0] = BodyGemm{"QKV projection", M, 3 * d, d, d, fp8};
    out[1] = BodyGemm{"up-projection", M, hid, d, d, fp8};
    out[2] = BodyGemm{"down projection", M, d, hid, hid, fp8};
    return 3;
}
inline bool body_gemm_fits(const BodyGemm& g) {
    GemmParams p{};
    p.M = g.M; p.N = g.N; p.K = g.K; p.lda = g.lda; p.ldw = g.K; p.f8 = g.f8 ? 1 : 0;
    return gemm_offsets_fit(p) != 0;
}

// ---- the training engine (tld_train_create): every refusal that is arithmetic on the configuration, in order; "" when it is good -----------------------------
// The transposing weight gradient (TLD_TRAIN_TN_WGRAD=0, and the fallback for widths that are no multiple of 256) feeds T1 / T2 -- [M + 4096 rows of
// max(hid, 3 d)] bf16, stacked split-K runs -- to launch_gemm: operand rows and the block-diagonal W offset stay inside that allocation, so the allocation
// below 4 GiB keeps every such launch inside the GEMM DMA's reach.  The rule implies the two GEMM A operands of M rows: the hidden activation [M, hid] and
// dqkv [M, 3 d].  Row chunks on a grid's y axis: the column sums (64-row chunks), the transposes (32-row tiles when M is no multiple of 64) and the depthwise
// weight gradient of the grids its fused backward does not take (one block per sample and image row).
inline std::string train_config_check(const tld_config& c) {
    if (c.embed_dim % 64 || c.embed_dim > 1024 || c.embed_dim <= 0) return "embed_dim must be a multiple of 64 (the head width), <= 1024";
    if (c.patch_size <= 0 || c.image_size % c.patch_size) return "image_size must be a multiple of patch_size";
    const int G = c.image_size / c.patch_size;
    // the inference engine's grids (square, side a multiple of 4: token counts that are multiples of 16, which the attention forward and
    // backward take), up to 64 x 64; the reference trains at whatever image_size it is given (tld/train.py:83)
    if (G % 4 || G < 4 || G > 64)
        return reach_say("the training step supports image_size / patch_size = G with G a multiple of 4, 4 <= G <= 64 (16 .. 4096 tokens); got G = %d", G);
    if (c.n_channels * c.patch_size * c.patch_size > 64) return "patch_dim must be <= 64";
    if (c.noise_embed_dims % 2 || c.max_batch <= 0 || c.n_layers <= 0 || c.mlp_multiplier <= 0) return "bad configuration";
    const uint64_t N = (uint64_t)G * G, d = (uint64_t)c.embed_dim, hid = d * c.mlp_multiplier, wide = hid > 3 * d ? hid : 3 * d;
    if (std::string bad = reach_refusal(c.max_batch, "the transposed weight-gradient operands T1 / T2", "(max_batch x tokens + 4096) x max(hidden width, 3 embed_dim) x 2 B",
                                        N * wide * 2, (uint64_t)kTrainTransposeMargin * wide * 2); !bad.empty()) return bad;
    // y axis: 64-row chunks of M rows (column sums) and of the M + 4096 rows of T1 / T2 (the 64 x 64 transpose); token counts that are no multiple of 64 can
    // make M one, and then the general transpose takes 32-row tiles of M rows
    const int64_t rows_fit = N % 64 ? kGridYZ * 32 : kGridYZ * 64 - kTrainTransposeMargin;
    if ((int64_t)N * c.max_batch > rows_fit)
        return reach_say("max_batch=%d: max_batch x tokens = %lld rows: the column-sum and transpose kernels put %s on the grid's y axis (at most %lld); the largest "
                         "max_batch that fits is %lld; run larger batches as several calls", c.max_batch, (long long)N * c.max_batch,
                         N % 64 ? "32-row tiles of them" : "64-row chunks of them and of 4096 rows more", (long long)kGridYZ, (long long)(rows_fit / (int64_t)N));
    if (!train_dw_fused(G, (int)N, (int)hid))
        return grid_refusal(c.max_batch, "max_batch x image_size / patch_size: the depthwise weight gradient puts one block per sample and image row on the grid's y axis", G);
    return std::string();
}

// ---- the CLIP towers (tld_clip_create, tld_clip_vis_create) ---------------------------------------------------------------------------------------------------
// rows per sample: context_length / tokens.  The MLP activation f [T, 4 W] bf16 is the largest GEMM A operand (T x 4 W < 2^31 also keeps every element index of
// the towers' row kernels inside an int); the image tower's patch matrix [max_batch x g x g, Kp] is wider than 4 W below width 768.
inline std::string clip_reach_check(int max_batch, int rows, int width, int patch_rows = 0, int patch_k = 0) {
    if (std::string bad = reach_refusal(max_batch, "the MLP activation", "max_batch x rows x 4 width x 2 B", (uint64_t)rows * 4 * width * 2); !bad.empty()) return bad;
    if (patch_rows) { if (std::string bad = reach_refusal(max_batch, "the patch matrix", "max_batch x patches x padded patch length x 2 B", (uint64_t)patch_rows * patch_k * 2); !bad.empty()) return bad; }
    return grid_refusal(max_batch, "the attention kernel puts one sample on each block of the grid's y axis", 1);
}

// ---- the raw-buffer test hooks: "" or the refusal (TLD_ERR_INVALID), before any allocation or launch -------------------------------------------------------------
// tld_debug_dwconv_gelu.  The row-streaming kernel (grid a multiple of 32) writes through 32-bit byte offsets from the buffer's base: batch x grid^2 x channels
// x 2 B must stay below 4 GiB.  The whole-image kernel (grid <= 16) and the tiled one (other grids) address in 64 bits and keep accepting; all three compute
// their workgroup count in an int.
inline std::string dwconv_hook_refusal(int batch, int grid, int channels) {
    const DwconvPlan w = plan_dwconv(batch, grid, channels, false);
    const uint64_t bytes = (uint64_t)batch * grid * grid * channels * 2;
    if (w.form == DW_STREAM && bytes >= kReach32)
        return reach_say("tld_debug_dwconv_gelu: batch %d x %d x %d tokens x %d channels = %llu bytes: the row-streaming kernel (grids that are multiples of 32) writes through "
                         "32-bit byte offsets and needs the buffer below 4 GiB; the largest batch that fits is %lld", batch, grid, grid, channels, (unsigned long long)bytes,
                         (long long)((kReach32 - 1) / ((uint64_t)grid * grid * channels * 2)));
    if (w.groups > kGridX)
        return reach_say("tld_debug_dwconv_gelu: %lld workgroups (batch %d, grid %d, %d channels) do not fit the launch's 32-bit count", (long long)w.groups, batch, grid, channels);
    return std::string();
}
// tld_debug_attention_fwd.  Every kernel addresses qk, vt and att in 64 bits: no size is refused for its bytes.  All but the chunked kernel (token counts that
// are multiples of 256 above 256) put the sample on the grid's z axis and the head on y.
inline std::string attention_fwd_hook_refusal(int batch, int ntok, int heads) {
    const AttentionPlan a = plan_attention(batch, ntok, heads);
    if (a.form != ATT_CHUNKED && (a.gz > kGridYZ || a.gy > kGridYZ))
        return reach_say("tld_debug_attention_fwd: batch %d, heads %d: at %d tokens the kernel puts heads and samples on the grid's y and z axes (at most %lld each)", batch, heads, ntok,
                         (long long)kGridYZ);
    if (a.form == ATT_CHUNKED && a.groups > kGridX)
        return reach_say("tld_debug_attention_fwd: batch %d x heads %d x %d query tiles do not fit the launch's 32-bit workgroup count", batch, heads, ntok / 256);
    return std::string();
}
// tld_debug_attention_bwd.  64-bit addressing throughout; one workgroup per (sample, head, block of at least 32 tokens), counted in an int.
inline std::string attention_bwd_hook_refusal(int batch, int ntok, int heads) {
    if ((int64_t)batch * heads * ((ntok + 31) / 32) > kGridX)
        return reach_say("tld_debug_attention_bwd: batch %d x heads %d x %d token blocks do not fit the launch's 32-bit workgroup count", batch, heads, (ntok + 31) / 32);
    return std::string();
}
// tld_debug_wgrad.  The transposing-read GEMM takes a 64-bit base per K-step and a 24-bit multiply of (row inside the step) x (row pitch in bytes): any number
// of rows, but n_out and k_in below 2^23 elements.
inline std::string wgrad_hook_refusal(int rows, int n_out, int k_in) {
    (void)rows;
    if (n_out >= (1 << 23) || k_in >= (1 << 23))
        return reach_say("tld_debug_wgrad: n_out %d, k_in %d: a row of either operand must stay below 2^24 bytes (the 24-bit multiply of the tile DMA)", n_out, k_in);
    return std::string();
}
// tld_debug_gemm_epilogue (and every other launch_gemm caller): the launch's own reach check, asked before the hook touches the device
inline std::string gemm_hook_refusal(const GemmParams& p) {
    return gemm_offsets_fit(p) ? std::string() : std::string(kGemmReachRefusal);
}

}  // namespace tld

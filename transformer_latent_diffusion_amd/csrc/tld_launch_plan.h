// tld_launch_plan.h -- the host decisions of the inference forward's row and attention launches (tld_rows.hip, tld_attn.hip): for
// every launch site the form, the template instantiation, the partition of the rows over workgroups, the grid, the dynamic LDS bytes and the launch-path
// bits the launch records.  A pure function of (sizes, which optional operands are given, CU count).  No HIP in this file:
// tests/host/launch_plan_main.cpp compiles it on its own and tests/test_launch_plan_host.py holds it against the restatement in tests/launch_plan_ref.py.
// Every rule is written ONCE here: the launchers make a plan, note its paths and switch on its form; tld_body_plan.h asks it which widths have a kernel
// and how much LDS the plain forms take; tld_reach.h asks it for the form and the workgroup count its hook refusals speak of.
#pragma once

#include <cstdint>

#include "tld_gemm_params.h"          // TLD_RESID_BF16

namespace tld {

// ---- launch-path record of the engine's stage hook (tld_engine_debug_paths; the table in include/tld_hip.h) -------------------------------
// Each bit is set by the launcher that launches the kernel, from the plan it launches by.  The sink is null unless a debug forward of an engine runs
// on this thread: with debug off a launch costs one thread-local load and a not-taken branch.
enum : int {
    EP_EMBED_PLAIN = 0, EP_EMBED_MFMA = 1 /* +0..3: TPW 2, 4, 6, 8 */, EP_LN_Q4 = 5 /* +0..3: q4<1..4> */, EP_LN_GENERIC = 9, EP_LN_MX8 = 10,
    EP_QKV_ATTN = 11, EP_QKV_LN = 12, EP_QKV_PLAIN = 13,
    EP_ATT_256 = 14, EP_ATT_CHUNKED = 15, EP_ATT_64 = 17 /* 18: unused (32 tokens: no square grid); 16: EP_TAIL_FOLD below */, EP_ATT_MASKED = 19,
    EP_CROSS_MFMA = 20 /* +0..3: NQ 1..4 */, EP_CROSS_GPW1 = 24, EP_CROSS_GPWN = 25, EP_CROSS_VALU = 26, EP_CROSS_FANOUT = 27,
    EP_UP_FUSED16 = 28, EP_UP_FUSED32_SEAM = 29, EP_UP_FUSED16_SMALL = 30, EP_UP_PLAIN = 31, EP_DW_WHOLE = 32, EP_DW_TILED = 33, EP_DW_STREAM = 34,
    EP_DOWN_STATS = 35, EP_DOWN_NOSTATS = 36, EP_DOWN_MAIN = 37, EP_DOWN_SMALL64 = 38, EP_DOWN_SMALL128 = 39,
    EP_SPLITK4 = 40, EP_SPLITK8 = 41, EP_SPLITK_SMALL = 42, EP_SPLITK_FINISH12 = 43, EP_SPLITK_FINISH6 = 44,
    EP_TAIL_MFMA = 45 /* +0..3: NT 1..4 */, EP_TAIL_PLAIN = 49, EP_UPDATE = 50, EP_UPDATE_FROM = 51, EP_UPDATE_FROM_MASK = 52, EP_START_MIX = 53,
    // fp8 GEMM mode, the writers of the MX-fp8 A operand (bit 10 is the quantising LayerNorm)
    EP_QUANT_MX8 = 54, EP_CROSS_F8 = 55, EP_DW_TILED_F8 = 56, EP_DW_STREAM_F8 = 57,
    // tld_sample_requests
    EP_UPDATE_REQ = 58, EP_UPDATE_REQ_MASK = 59, EP_START_MIX_REQ = 60,
    // out_proj folded into the last block's down projection (bit 16 was unused): set next to the EP_TAIL_MFMA bit of the launch's patch-feature tiles
    EP_TAIL_FOLD = 16,
    // fused QKV + attention on two-head tiles (EPI_QKV_ATTN2); a launch sets this bit INSTEAD of EP_QKV_ATTN
    EP_QKV_ATTN_PAIR = 61,
    // the step of a sampler session (tld_session_step)
    EP_UPDATE_SESSION = 62,
    EP_COUNT = 63
};
constexpr uint64_t ep_bit(int bit) { return 1ull << bit; }

#ifdef TLD_RESID_BF16
constexpr bool kResidBf16 = true;
#else
constexpr bool kResidBf16 = false;    // the matrix-pipe embed and tail, the folds and the fp8 mode feed the bf16 residual stream straight to the MFMA: none of them in the fp32-residual build
#endif

#ifndef TLD_ATTN_ST16
#define TLD_ATTN_ST16 2       // 256-token kernel's output stores: 2 = whole 128-byte rows via an LDS transpose, 1 = 16-byte stores after a lane-pair exchange, 0 = 8-byte stores
#endif

constexpr int kLdsLimit = 160 * 1024;             // LDS of a CU: what a workgroup's dynamic LDS can be opted in to
constexpr int kDwChannels = 64;                   // channels per workgroup of the depthwise kernels

// What every plan carries: the grid and the block, the workgroup count in 64 bits (the extents are its truncation, as the launchers' casts were), the dynamic
// LDS bytes and the launch-path bits.
struct LaunchGeom {
    uint32_t gx = 1, gy = 1, gz = 1, block = 0;
    int64_t groups = 0;
    int lds = 0;
    uint64_t paths = 0;
};
inline void geom_rows(LaunchGeom& g, int64_t groups, int block) { g.groups = groups; g.gx = (uint32_t)groups; g.block = (uint32_t)block; }

// d = 64 k (k = 1 .. 16) in the row kernels that hold a token row in 128-feature register groups: NJ = ceil(d / 128) groups per lane, HALF when the last one
// holds 64 features
inline int row_nj(int d) { return (d + 127) / 128; }
inline bool row_half(int d) { return d % 128 != 0; }

// ---- the LDS of the plain forms: what body_config_check (tld_body_plan.h) holds against the limit -----------------------------------------------------------
inline int embed_plain_lds(int pd, int cpp, int d) { return (pd * d + pd * cpp) * 4; }             // Linear weight [pd][d], conv weight [pd][C p p]
inline int tail_plain_lds(int pd, int d) { return pd * d * 4; }                                    // out_proj weight [pd][d]
inline int cross_row_valu_lds(int d, int heads) { return (heads * d + 2 * d + heads) * 4; }        // query-difference table, the two value rows, the logit biases

// ---- embed (launch_embed) ----------------------------------------------------------------------------------------------------------------------------------
// `cpp`: n_channels x patch_size^2, the conv's input patch (the engine's pd).  `held`: the split-bf16 image of the Linear weight (lin_w_hl) is given.
enum EmbedForm { EMBED_PLAIN, EMBED_MFMA };
struct EmbedPlan : LaunchGeom { EmbedForm form = EMBED_PLAIN; int tpw = 0, nj = 0; bool half = false; };
inline EmbedPlan plan_embed(int batch, int ntok, int pd, int cpp, int d, bool held) {
    EmbedPlan p;
    geom_rows(p, ((int64_t)batch * ntok + 31) / 32, 256);                   // 32 token rows per workgroup
    if (kResidBf16 && held && pd == 16 && cpp == 16 && d % 256 == 0 && d <= 1024) {       // matrix-pipe form
        p.form = EMBED_MFMA; p.tpw = d / 128;
        p.lds = 16 * 16 * 4 + 4 * 4 * 32 * 4 + 3 * d * 4 + 4 * 32 * 144;    // conv weight, row partials, bias / LayerNorm vectors, transpose patches
        p.paths = ep_bit(EP_EMBED_MFMA + d / 256 - 1);
        return p;
    }
    p.nj = row_nj(d); p.half = row_half(d);
    p.lds = embed_plain_lds(pd, cpp, d);
    p.paths = ep_bit(EP_EMBED_PLAIN);
    return p;
}

// ---- LayerNorm-1 (launch_layernorm_bf16, launch_layernorm_mx8) ----------------------------------------------------------------------------------------------
// One wave per row, four rows per workgroup.  The four-features-per-lane kernels exist at d = 256 k; the quantising one (`mx8`: MX-fp8 codes and scales
// instead of bf16) at 256, 512 and 768 only -- at any other width there is NO SUCH KERNEL: LN_NONE, which the engine's mode never reaches (plan_body asks
// layernorm_mx8_supported before it sets ln_mx8; tests/test_launch_plan_host.py holds that over the whole body-plan sweep).
enum LnForm { LN_NONE, LN_Q4, LN_GENERIC, LN_MX8 };
struct LayerNormPlan : LaunchGeom { LnForm form = LN_NONE; int nq = 0, nj = 0; bool half = false; };
inline LayerNormPlan plan_layernorm(int M, int d, bool mx8) {
    LayerNormPlan p;
    geom_rows(p, ((int64_t)M + 3) / 4, 256);
    const bool q4 = d == 256 || d == 512 || d == 768 || d == 1024;
    if (mx8) {
        p.paths = ep_bit(EP_LN_MX8);
        if (q4 && d != 1024) { p.form = LN_MX8; p.nq = d / 256; }
    } else if (q4) {
        p.form = LN_Q4; p.nq = d / 256; p.paths = ep_bit(EP_LN_Q4 + d / 256 - 1);
    } else {
        p.form = LN_GENERIC; p.nj = row_nj(d); p.half = row_half(d); p.paths = ep_bit(EP_LN_GENERIC);
    }
    return p;
}
inline bool layernorm_mx8_supported(int d) { return plan_layernorm(1, d, true).form == LN_MX8; }

// ---- cross_row (launch_cross_row) -------------------------------------------------------------------------------------------------------------------------
// `x_in`: the fan-out input of a shared layer 0 is given.  `f8`: the MX-fp8 output (xn3_f8) is asked for.
enum CrossForm { CROSS_VALU, CROSS_MFMA };
struct CrossRowPlan : LaunchGeom {
    CrossForm form = CROSS_VALU;
    int nq = 0, gpw = 0;                 // matrix-pipe form: d / 256; 16-row groups per workgroup
    int nj = 0, cps = 0; bool half = false;      // VALU form: feature groups per lane; chunks per sample
    bool mode_outputs = false;           // the LN3-statistics output (CrossRowParams::ln3_stats) and the MX-fp8 one: what the engine's mode may ask of this width
};
inline CrossRowPlan plan_cross_row(int batch, int ntok, int d, int heads, bool x_in, bool f8, int cus) {
    CrossRowPlan p;
    if (d % 256 == 0 && d <= 1024 && ntok % 16 == 0) {
        // 512-thread workgroups over 16-row groups of one sample, ONE per CU (the kernel holds ~170 registers at d = 768: the split-bf16 slices of
        // the query-difference vectors and the prefetched row pair live in registers; two workgroups per CU at 128 registers spilled and ran
        // 43.7 us against 38.0).  Groups per workgroup: the largest power of two (<= 16) that divides a sample's groups and still leaves >= 1
        // workgroup per CU (at C1: 128 samples x 16 groups / 8 = 256 workgroups = one resident round)
        p.form = CROSS_MFMA; p.nq = d / 256;
        const int gps = ntok / 16;
        int gpw = 1;
        while (gpw < 16 && gps % (gpw * 2) == 0 && (int64_t)batch * (gps / (gpw * 2)) >= cus) gpw *= 2;
        p.gpw = gpw;
        p.mode_outputs = d != 1024;      // both outputs exist in the matrix-pipe kernel only; the mode takes them at 256, 512 and 768 (kept as it was)
        p.lds = 2 * 16 * d * 2 + 8 * 256 * 4 + 2 * d * 4;      // split-bf16 tile, partial logits, the two value rows
        geom_rows(p, (int64_t)batch * (gps / gpw), 512);
        p.paths = ep_bit(EP_CROSS_MFMA + d / 256 - 1) | ep_bit(gpw > 1 ? EP_CROSS_GPWN : EP_CROSS_GPW1) | (x_in ? ep_bit(EP_CROSS_FANOUT) : 0) | (f8 ? ep_bit(EP_CROSS_F8) : 0);
        return p;
    }
    // other widths (any multiple of 64): the 2-features-per-lane VALU kernel.  ~43 KB of LDS per workgroup -> 3 workgroups per CU.  Split each
    // sample's row pairs into the number of chunks that makes the grid ONE full resident round (768 workgroups on 256 CUs) when the batch
    // allows, else k rounds of <= ~48 rows per workgroup; a partial extra round costs as much as a full one.
    const int64_t slots = 3 * (int64_t)cus, rows = (int64_t)batch * ntok;
    const int64_t k = (rows + slots * 48 - 1) / (slots * 48);
    int64_t cps = slots * k / batch;
    const int64_t max_cps = ntok / 8 > 0 ? ntok / 8 : 1;          // at least one row pair per wave
    if (cps > max_cps) cps = max_cps;
    if (cps < 1) cps = 1;
    p.cps = (int)cps; p.nj = row_nj(d); p.half = row_half(d);
    p.lds = cross_row_valu_lds(d, heads);
    geom_rows(p, (int64_t)batch * cps, 256);
    p.paths = ep_bit(EP_CROSS_VALU) | (x_in ? ep_bit(EP_CROSS_FANOUT) : 0);
    return p;
}
// which widths write LN3 statistics, or LN3(x) as the MX-fp8 operand of the up-projection
inline bool cross_row_supports_ln3_stats(int d) { return plan_cross_row(1, 16, d, d / 64, false, false, 1).mode_outputs; }

// ---- the split-K finish of the low-latency down projection (launch_splitk_resid) ------------------------------------------------------------------------------
// One wave per row, lane l owns CPL = d / 64 columns; a 96-column statistics group must be a power-of-two run of lanes: d = 768 and 384.  Any other width:
// no such kernel (body_class_refusal refuses the class there).
enum SplitkFinishForm { SKF_NONE, SKF_CPL12, SKF_CPL6 };
struct SplitkFinishPlan : LaunchGeom { SplitkFinishForm form = SKF_NONE; int cpl = 0; };
inline SplitkFinishPlan plan_splitk_finish(int M, int d) {
    SplitkFinishPlan p;
    geom_rows(p, ((int64_t)M + 3) / 4, 256);
    if (d == 768) { p.form = SKF_CPL12; p.cpl = 12; p.paths = ep_bit(EP_SPLITK_FINISH12); }
    else if (d == 384) { p.form = SKF_CPL6; p.cpl = 6; p.paths = ep_bit(EP_SPLITK_FINISH6); }
    return p;
}
inline bool splitk_resid_supported(int d) { return plan_splitk_finish(1, d).form != SKF_NONE; }

// ---- the tail (launch_tail) ---------------------------------------------------------------------------------------------------------------------------------
// `hid`: the last block's hidden activation is given (the folded form: tok = x2, hid = hid2, any d and any hidden width: both are multiples of 64).
// `held`: the split-bf16 image of the out_proj weight (w_hl) is given.
enum TailForm { TAIL_PLAIN, TAIL_MFMA, TAIL_FOLD };
struct TailPlan : LaunchGeom {
    TailForm form = TAIL_PLAIN;
    int nt = 0, rt = 0;                  // matrix-pipe forms: 16-feature tiles of the patch (1 .. 4); folded form: 16-row tiles per workgroup (1, or 4 / 2)
    int nj = 0, rows_per_block = 0; bool half = false;      // plain form
};
inline TailPlan plan_tail(int batch, int ntok, int pd, int d, bool hid, bool held, int cus) {
    TailPlan p;
    const int64_t rows = (int64_t)batch * ntok;
    const int nt = (pd + 15) / 16, ntc = nt < 4 ? nt : 4;
    if (kResidBf16 && hid) {
        // row tiles per workgroup: as many as keep a fragment's re-use high while every CU still has a workgroup; LDS 8 RT NT KiB <= 64 KiB
        const int big = nt <= 2 ? 4 : 2;
        p.form = TAIL_FOLD; p.nt = ntc; p.rt = rows >= 16 * (int64_t)big * cus ? big : 1;
        p.lds = 8 * p.rt * nt * 1024;
        geom_rows(p, (rows + 16 * p.rt - 1) / (16 * p.rt), 512);
        p.paths = ep_bit(EP_TAIL_MFMA + ntc - 1) | ep_bit(EP_TAIL_FOLD);
        return p;
    }
    if (kResidBf16 && held && d % 128 == 0 && (int64_t)pd * d <= 40960) {      // matrix-pipe form: split-bf16 weights [2][pd][d] in <= 160 KiB of LDS (the XOR swizzle of its
                                                                                // weight image permutes 16-byte chunks within aligned groups of 16: rows of d / 8 = 16 k chunks)
        p.form = TAIL_MFMA; p.nt = ntc;
        p.lds = 2 * nt * 16 * d * 2;
        geom_rows(p, (rows + 63) / 64, 256);
        p.paths = ep_bit(EP_TAIL_MFMA + ntc - 1);
        return p;
    }
    p.rows_per_block = 64; p.nj = row_nj(d); p.half = row_half(d);
    p.lds = tail_plain_lds(pd, d);
    geom_rows(p, (rows + p.rows_per_block - 1) / p.rows_per_block, 256);
    p.paths = ep_bit(EP_TAIL_PLAIN);
    return p;
}

// ---- depthwise conv + GELU (launch_dwconv_gelu) -----------------------------------------------------------------------------------------------------------
// `grid`: tokens per side.  `f8`: the MX-fp8 output is asked for (the streaming and the tiled kernel write it; the whole-image kernel writes bf16 only).
enum DwForm { DW_WHOLE, DW_TILED, DW_STREAM };
struct DwconvPlan : LaunchGeom { DwForm form = DW_WHOLE; bool f8 = false; };
inline DwconvPlan plan_dwconv(int batch, int grid, int channels, bool f8) {
    DwconvPlan p;
    const int64_t chunks = channels / kDwChannels;
    if (grid > 16 && grid % 32 == 0) {       // row-streaming variant (ring of image rows in LDS, a DMA wave): 32-column strips; halved tables
        p.form = DW_STREAM; p.f8 = f8;
        geom_rows(p, (int64_t)batch * (grid / 32) * chunks, 320);
        p.paths = ep_bit(EP_DW_STREAM) | (f8 ? ep_bit(EP_DW_STREAM_F8) : 0);
    } else if (grid > 16) {                  // spatially tiled variant (halo in LDS): 16 x 16 tiles, the last ones partial; halved tables
        const int64_t tiles = (grid + 15) / 16;
        p.form = DW_TILED; p.f8 = f8;
        geom_rows(p, (int64_t)batch * tiles * tiles * chunks, 256);
        p.paths = ep_bit(EP_DW_TILED) | (f8 ? ep_bit(EP_DW_TILED_F8) : 0);
    } else {                                 // the whole image of a (sample, channel chunk) in LDS
        p.lds = grid * grid * 128;
        geom_rows(p, (int64_t)batch * chunks, 256);
        p.paths = ep_bit(EP_DW_WHOLE);
    }
    return p;
}

// ---- self-attention (launch_attention) ----------------------------------------------------------------------------------------------------------------------
// 256 tokens: two unsynchronised 4-wave workgroups per CU, each staging its (sample, head)'s K / V^T once (attn1_kernel; the single 8-wave workgroup it
// replaced took 60 us against 44 at C1).  Other multiples of 256: the chunked two-query-tile kernel (attn2_kernel), workgroups on x alone.  128, 64 and 32
// tokens: attn_kernel<KT, NW> with the whole sample in one chunk of KT x 32 keys.  Any other multiple of 8 (tld_engine_create checks): the masked kernel,
// 128-key chunks, 4-wave workgroups of 128 queries, partial last chunk / block masked.
// (At the C1 shape the inference engine no longer comes here: its self-attention runs in the QKV GEMM's epilogue, EPI_QKV_ATTN.)
// (128 and 32 tokens carry no launch-path bit: no square token grid has them, only tld_debug_attention_fwd comes here with those counts.)
enum AttnForm { ATT_256, ATT_CHUNKED, ATT_ONE_CHUNK, ATT_MASKED };
struct AttentionPlan : LaunchGeom { AttnForm form = ATT_MASKED; int kt = 0, nw = 0, nbuf = 1; int64_t npairs = 0; };
inline int attn_stage_lds(int kc) { return kc * 128 + 64 * (kc * 2 + 8); }      // one K chunk [kc][64] and one V^T chunk [64][kc + pad] in bf16
inline AttentionPlan plan_attention(int batch, int ntok, int heads) {
    AttentionPlan p;
    auto chunks = [&](int kt, int nw, int64_t qblocks) {      // attn_kernel: a second buffer where there is a second chunk to stage under the first (and LDS for it)
        p.kt = kt; p.nw = nw;
        p.nbuf = (ntok > kt * 32 && 2 * attn_stage_lds(kt * 32) <= kLdsLimit) ? 2 : 1;
        p.lds = p.nbuf * attn_stage_lds(kt * 32);
        p.gx = (uint32_t)qblocks; p.gy = (uint32_t)heads; p.gz = (uint32_t)batch; p.block = (uint32_t)(nw * 64);
        p.groups = qblocks * heads * batch;
    };
    if (ntok == 256) {
        p.form = ATT_256; p.kt = 8; p.nw = 4;
        p.lds = attn_stage_lds(256) + (TLD_ATTN_ST16 == 2 ? p.nw * 16 * 144 : 0);
        p.gy = (uint32_t)heads; p.gz = (uint32_t)batch; p.block = 256; p.groups = (int64_t)heads * batch;
        p.paths = ep_bit(EP_ATT_256);
    } else if (ntok % 256 == 0) {
        p.form = ATT_CHUNKED;
        p.lds = 2 * 128 * 128 + 2 * 64 * 256 + 4 * 16 * 144;
        p.npairs = (int64_t)batch * heads;
        geom_rows(p, ((p.npairs + 7) / 8) * 8 * (ntok / 256), 256);         // pairs padded to whole rounds of the 8 XCDs (the surplus workgroups return at once)
        p.paths = ep_bit(EP_ATT_CHUNKED);
    } else if (ntok == 128) { p.form = ATT_ONE_CHUNK; chunks(4, 4, 1); }
    else if (ntok == 64) { p.form = ATT_ONE_CHUNK; chunks(2, 2, 1); p.paths = ep_bit(EP_ATT_64); }
    else if (ntok == 32) { p.form = ATT_ONE_CHUNK; chunks(1, 1, 1); }
    else { p.form = ATT_MASKED; chunks(4, 4, ((int64_t)ntok + 127) / 128); p.paths = ep_bit(EP_ATT_MASKED); }
    return p;
}

}  // namespace tld

// tld_body_plan.h -- the mode of an inference engine (tld_engine.hip): which of the forward's structural paths it takes, which
// weight images and buffers it therefore holds, which stages its hook reserves, and every refusal of tld_engine_create, tld_engine_set_low_latency and
// tld_engine_set_gemm_dtype that is arithmetic on the configuration.  A pure function of (configuration, switches, operand type, low-latency class,
// max_batch, CU count).  No HIP in this file: tests/host/body_plan_main.cpp compiles it on its own and tests/test_body_plan_host.py holds it against
// the restatement in tests/body_plan_ref.py.  Every rule is written ONCE here; tld_engine.hip reads the fields.
#pragma once

#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tld_hip.h"
#include "tld_gemm_plan.h"            // gemm_resid_stat_slots, kLnSlots, bf16, resid_t
#include "tld_launch_plan.h"          // kResidBf16; which widths the row kernels have (layernorm_mx8_supported, cross_row_supports_ln3_stats, splitk_resid_supported) and their LDS
#include "tld_qkv_pair_plan.h"        // plan_qkv_pair
#include "tld_reach.h"                // body_reach_check: the sizes the kernels' 32-bit offsets and 16-bit grid axes end at
#include "tld_stages.h"               // ST_*: the element types of the stage hook
#include "tld_tail_fold_math.h"       // tail_fold_padded_rows

namespace tld {

// ---- the derived shape of a configuration (after body_config_check) ------------------------------------------------------------------------------------------
struct BodyShape { int d, L, H, grid, ntok, pd, hid, img, ne, text; };
inline BodyShape body_shape(const tld_config& c) {
    BodyShape s{};
    s.d = c.embed_dim; s.L = c.n_layers; s.H = c.embed_dim / 64; s.grid = c.image_size / c.patch_size; s.ntok = s.grid * s.grid;
    s.pd = c.n_channels * c.patch_size * c.patch_size; s.hid = c.mlp_multiplier * c.embed_dim; s.img = c.n_channels * c.image_size * c.image_size;
    s.ne = c.noise_embed_dims; s.text = c.text_emb_size;
    return s;
}

inline std::string body_say(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
inline std::string body_say(const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof b, fmt, ap);
    va_end(ap);
    return b;
}

// The refusals of tld_engine_create on the configuration, in order; "" when it is good.  `ndev` is the device count; < 0: not known yet, and the answer covers
// the refusals in front of the device_id one only.  (The architecture check stays with the caller.)
inline std::string body_config_check(const tld_config& c, int ndev) {
    if (c.embed_dim <= 0 || c.embed_dim % 64 != 0 || c.embed_dim > 1024)
        return body_say("embed_dim=%d unsupported: must be a multiple of the head width 64 (n_heads = embed_dim // 64, "
                        "tld/transformer_blocks.py:126-128) and <= 1024 (the row kernels hold a token row in 8 x 128-feature register groups)", c.embed_dim);
    if (c.patch_size <= 0 || c.image_size % c.patch_size != 0) return body_say("image_size=%d must be divisible by patch_size=%d", c.image_size, c.patch_size);
    const int grid = c.image_size / c.patch_size, ntok = grid * grid;
    // any grid whose side is a multiple of 4 (token count a multiple of 16: the 16-row groups of the cross-attention row kernel, 16-byte V^T
    // rows); 64 / 128 / k 256 tokens have shape-specialised attention kernels, everything else takes the masked chunked one
    if (ntok % 16 != 0) return body_say("token count %d unsupported: image_size / patch_size must be a multiple of 4", ntok);
    const int pd = c.n_channels * c.patch_size * c.patch_size;
    if (pd > 64) return body_say("patch_dim=%d > 64 unsupported", pd);
    if (c.noise_embed_dims % 2 || c.noise_embed_dims <= 0) return "noise_embed_dims must be even";
    if (c.max_batch <= 0 || c.n_layers <= 0 || c.mlp_multiplier <= 0 || c.text_emb_size <= 0) return "non-positive size in config";
    if ((c.mlp_multiplier * c.embed_dim) % 64) return "hidden width must be a multiple of 64";
    // the GEMM tile DMA addresses operands with 32-bit byte offsets
    const int64_t hid_bytes = (int64_t)c.max_batch * grid * grid * c.mlp_multiplier * c.embed_dim * 2;
    if (hid_bytes >= (int64_t)1 << 32)
        return body_say("max_batch=%d: the hidden activation (%lld bytes) must stay below 4 GiB; run larger batches as several calls", c.max_batch, (long long)hid_bytes);
    // ... and what that rule alone does not hold: q|k at mlp_multiplier 1, the samples on the attention kernels' z axis
    if (std::string bad = body_reach_check(c, grid); !bad.empty()) return bad;
    if (ndev < 0) return std::string();
    if (c.device_id < 0 || c.device_id >= ndev) return body_say("device_id %d out of range (%d devices)", c.device_id, ndev);
    // the row kernels keep per-workgroup tables in dynamic LDS (opted in above the 64-KiB default; a CU has 160 KiB)
    const int d = c.embed_dim;
    const long embed_lds = embed_plain_lds(pd, pd, d), tail_lds = tail_plain_lds(pd, d), cross_lds = cross_row_valu_lds(d, d / 64), lim = kLdsLimit;      // the plain forms'
    if (embed_lds > lim || tail_lds > lim || cross_lds > lim)
        return body_say("embed_dim=%d with patch_dim=%d needs %ld / %ld / %ld bytes of LDS in the embed / out-proj / cross-attention row kernels (limit %ld each): "
                        "reduce patch_size*patch_size*n_channels or embed_dim", c.embed_dim, pd, embed_lds, tail_lds, cross_lds, lim);
    return std::string();
}

// ---- the switches: read once, at tld_engine_create (A/B testing; every one defaults to the fast path) ------------------------------------------------------
struct BodySwitches {
    bool fold_ln1 = true;          // TLD_FOLD_LN1=0: separate LayerNorm-1 kernel
    bool fold_ln3 = true;          // TLD_FOLD_LN3=0: cross_row writes LN3(x) and the up-projection reads it
    bool fold_tail = true;         // TLD_FOLD_TAIL=0: the last block's down projection and out_proj stay two kernels
    bool fuse_dwconv = true;       // TLD_FUSE_DWCONV=0: up-projection and depthwise conv + GELU as two kernels
    bool fuse_qkv_attn = true;     // TLD_FUSE_QKV_ATTN=0: QKV GEMM and self-attention as two kernels
    bool fp8_fused = true;         // TLD_FP8_FUSED=0: separate quantisation passes instead of quantising producers
    int qkv_pair = 1;              // TLD_QKV_ATTN_PAIR: the fused QKV + attention kernel on two-head tiles: 0 never, 1 where plan_qkv_pair says so, 2 wherever the shape permits (test hook)
    bool share_l0 = true;          // TLD_SHARE_L0=0: no layer-0 sharing between the halves of a CFG-doubled batch
    bool guidance_skip = true;     // TLD_GUIDANCE_SKIP=0: tld_sample_requests_guided runs the unconditional sample of an unguided step too
};
// `get(name)` is getenv-like: the value, or null.  atoi semantics: a value that is no number is 0, which is off.
template <class Get>
inline BodySwitches body_switches(Get get) {
    BodySwitches s;
    auto flag = [&get](const char* name, bool* v) { if (const char* t = get(name)) *v = atoi(t) != 0; };
    flag("TLD_FOLD_LN1", &s.fold_ln1); flag("TLD_FOLD_LN3", &s.fold_ln3); flag("TLD_FOLD_TAIL", &s.fold_tail); flag("TLD_FUSE_DWCONV", &s.fuse_dwconv);
    flag("TLD_FUSE_QKV_ATTN", &s.fuse_qkv_attn); flag("TLD_FP8_FUSED", &s.fp8_fused); flag("TLD_SHARE_L0", &s.share_l0); flag("TLD_GUIDANCE_SKIP", &s.guidance_skip);
    if (const char* t = get("TLD_QKV_ATTN_PAIR")) { const int v = atoi(t); s.qkv_pair = v < 0 ? 0 : v > 2 ? 2 : v; }
    return s;
}
// What tld_engine_set_gemm_dtype does to the switches.  KEPT AS IT WAS, on purpose: (1) writes the two folds and the fused depthwise epilogue off and (0) does
// not put them back, so "1 then 0" before finalize leaves a bf16 engine without them.  Only the ABI error-path test does that, on an engine it destroys at once.
inline void body_switches_set_dtype(BodySwitches& s, int dtype) { if (dtype == 1) s.fold_ln1 = s.fold_ln3 = s.fuse_dwconv = false; }

// ---- the refusals of the two setters, in order; "" when the request is good ---------------------------------------------------------------------------------
// K-splits of the low-latency down projection: class 1 = four (engines of at most 4096 token rows), class 2 = eight (at most 1024 token rows: one or two images per CFG call,
// the one-prompt-per-call pattern).  Eight splits take a one-image generate from 36.4 to 33.4 ms, but cost 6-8 ms at four or five images (twice the work items of 6 K-steps
// each no longer fit one round of workgroups, and the finishing kernel reads twice the slices) -- hence two classes, each chosen by the CALLER for the engine and each with its
// own fp32 summation order: inside a class results are bit-identical across batch sizes.
constexpr int kLowLatMaxRows2 = 1024;       // class 2 (eight K-splits): one or two images per CFG call
constexpr int kLowLatMaxRows = 4096;        // class 1 (four): capacity in token rows = max_batch x tokens; beyond it the tiles fill the chip by themselves
inline int lowlat_split(int cls) { return cls == 2 ? 8 : cls == 1 ? 4 : 0; }
inline std::string body_class_refusal(const BodyShape& s, int max_batch, int cls, bool fp8) {
    if (!cls) return std::string();
    if (cls != 1 && cls != 2) return body_say("low-latency class %d: 0 = off, 1 = four K-splits (engines up to %d token rows), 2 = eight (up to %d)", cls, kLowLatMaxRows, kLowLatMaxRows2);
    if (fp8) return "low-latency class: bf16 GEMM operands only -- this engine runs MX-fp8 GEMMs (tld_engine_set_gemm_dtype), whose down projection has no split-K form";
    const int64_t rows = (int64_t)max_batch * s.ntok;
    const int max_rows = cls == 2 ? kLowLatMaxRows2 : kLowLatMaxRows;
    if (rows > max_rows)
        return body_say("low-latency class %d: engine capacity %lld token rows (max_batch %d x %d tokens) exceeds %d -- at that size %s", cls, (long long)rows, max_batch, s.ntok,
                        max_rows, cls == 2 ? "class 1 (four K-splits) is the faster one" : "the default tiles fill the chip");
    const int split = lowlat_split(cls);
    if (!splitk_resid_supported(s.d) || s.hid % (64 * split) != 0)
        return body_say("low-latency class: needs embed_dim 384 or 768 (got %d) and a hidden width that splits into %d multiples of 64 (got %d)", s.d, split, s.hid);
    return std::string();
}
inline std::string body_dtype_refusal(const BodyShape& s, int dtype, int cls) {
    if (dtype != 0 && dtype != 1) return body_say("gemm dtype %d: 0 = bf16, 1 = MX-fp8 (e4m3 + E8M0 block scales)", dtype);
    if (dtype == 0) return std::string();
    if (cls) return "fp8 GEMMs and the low-latency class exclude each other (the split-K down projection is bf16 only): clear tld_engine_set_low_latency first";
    if (!kResidBf16) return "the fp8 GEMM mode exists in the bf16-residual build only";
    if (s.d % 128 || s.hid % 128) return "fp8 GEMMs need embed_dim and hidden width multiples of 128";
    return std::string();
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------------------------------------
struct BodyPlan {
    bool fp8 = false; int cls = 0, heads = 0, cus = 0;      // the inputs the launches ask about again
    bool share_l0 = true, guidance_skip = true;             // the two switches that are no structure of the body: offered to the calls as they are
    bool fold_ln1 = false;         // LayerNorm-1 applied inside the QKV GEMM's epilogue: needs the down projection's 96-column partial sums (d % 192 == 0, at most 8 groups) and
                                   // a QKV width the 256-wide kernel takes for every batch size
    bool fold_ln3 = false;         // LayerNorm-3 applied in the up-projection's epilogue: needs the statistics-writing row kernel
    bool fused_qa = false;         // QKV GEMM + self-attention as ONE kernel per (sample, head): 256-token samples, the LayerNorm-1 fold (the kernel reads the raw residual
                                   // stream) and an even number of 64-wide K-steps (its LDS map relies on which stage a tile consumes last); bf16 only
    bool pair_held = false;        // ... its head-pair images and slots are held: heads even, the switch not 0, no low-latency class AT FINALIZE, and a batch <= max_batch takes them
    bool pair = false;             // ... and a launch may take them: held, and no low-latency class NOW (which launch does: body_pair_launch)
    bool pair_always = false;      // TLD_QKV_ATTN_PAIR=2
    int64_t pair_slots = 0;        // workgroups such a launch can have: min(head pairs of max_batch, CUs)
    bool fuse_dw = false;          // depthwise conv + GELU inside the up-projection's epilogue: 16 x 16 tokens (a tile row-block is one image) or 32 x 32 (8 image rows) ...
    bool seam = false;             // ... where a thin second kernel finishes the two rows at every tile seam from the seam buffer
    bool fold_tail_held = false;   // [Wout | Wout Wd] is held: bf16 operands
    bool fold_tail = false;        // ... and the last block's down projection runs inside the tail: no low-latency class (its split-K form is that GEMM)
    bool ln_mx8 = false, cross_mx8 = false, dw_mx8 = false;              // fp8: LayerNorm-1 / cross_row / the depthwise kernel write the MX8 operand of the next GEMM themselves
    bool quant_qkv = false, quant_up = false, quant_down = false;        // ... or a separate quant pass does: exactly one of the two per operand
    int ll_split = 0;              // K-splits of the low-latency down projection (0: the plain GEMM)
};

// `finalized`: the plan the engine allocated its images from.  What is held stays as it was then; a class set or cleared later only changes what a launch does with it.
inline BodyPlan plan_body(const BodyShape& s, const BodySwitches& sw, bool fp8, int cls, int max_batch, int cus, const BodyPlan* finalized = nullptr) {
    BodyPlan p;
    p.fp8 = fp8; p.cls = cls; p.heads = s.H; p.cus = cus; p.share_l0 = sw.share_l0; p.guidance_skip = sw.guidance_skip;
    const bool bf = !fp8 && kResidBf16;     // (fp8: activations are quantised from the separately written LayerNorm / GELU outputs: no folds, no fused depthwise epilogue)
    p.fold_ln1 = sw.fold_ln1 && bf && gemm_resid_stat_slots(s.d) > 0 && (3 * s.d) % 256 == 0;
    p.fold_ln3 = sw.fold_ln3 && bf && s.hid % 256 == 0 && cross_row_supports_ln3_stats(s.d);
    p.fused_qa = sw.fuse_qkv_attn && p.fold_ln1 && s.ntok == 256 && s.d % 128 == 0;
    p.pair_always = sw.qkv_pair == 2;
    if (finalized) p.pair_held = finalized->pair_held;
    else if (p.fused_qa && !cls && s.H % 2 == 0 && sw.qkv_pair != 0) {
        p.pair_held = p.pair_always;
        for (int b = 1; b <= max_batch && !p.pair_held; ++b) p.pair_held = plan_qkv_pair(b, s.H, cus);
    }
    p.pair = p.pair_held && p.fused_qa && !cls;
    const int64_t pairs = (int64_t)max_batch * (s.H / 2);
    p.pair_slots = p.pair_held ? (pairs < cus ? pairs : cus) : 0;
    p.fuse_dw = sw.fuse_dwconv && !fp8 && (s.grid == 16 || s.grid == 32) && s.hid % 256 == 0;
    p.seam = p.fuse_dw && s.grid == 32;
    p.fold_tail_held = sw.fold_tail && bf;
    p.fold_tail = p.fold_tail_held && !cls;
    const bool fuse8 = fp8 && sw.fp8_fused;
    p.ln_mx8 = fuse8 && layernorm_mx8_supported(s.d);
    p.cross_mx8 = fuse8 && cross_row_supports_ln3_stats(s.d);      // (= the 4-features-per-lane kernel is in use)
    p.dw_mx8 = fuse8 && s.grid > 16;                                // the tiled and streaming kernels; the whole-image one of 16 x 16 tokens writes bf16
    p.quant_qkv = fp8 && !p.ln_mx8; p.quant_up = fp8 && !p.cross_mx8; p.quant_down = fp8 && !p.dw_mx8;
    p.ll_split = fp8 ? 0 : lowlat_split(cls);
    return p;
}
// two heads per tile for a launch of `samples` samples (the same bits either way)
inline bool body_pair_launch(const BodyPlan& p, int samples) { return p.pair && (p.pair_always || plan_qkv_pair(samples, p.heads, p.cus)); }

// ---- one decoder block's weight images --------------------------------------------------------------------------------------------------------------------------
// As tld_engine_finalize_weights allocates them for the engine's mode (a null pointer: not held in this mode).  Plain pointers only: finalize keeps a device copy
// of the engine's array of these, and the refresh kernels (tld_refresh.hip) index it by blockIdx.z.
struct Layer {
    bf16 *qkv_w = nullptr, *up_w = nullptr, *down_w = nullptr;
    bf16 *qkv_wf = nullptr;                               // bf16(gamma1 (.) Wqkv): LayerNorm-1 folded into the QKV GEMM
    float *qkv_c1 = nullptr, *qkv_b1 = nullptr;           // [3d] column sums of qkv_wf; beta1 . Wqkv^T
    bf16 *qkv_wp = nullptr;                               // qkv_wf with its rows permuted to [head][q_h | k_h | v_h] (fused QKV -> attention kernel)
    float *qkv_c1p = nullptr, *qkv_b1p = nullptr;         // the same permutation of qkv_c1 / qkv_b1
    bf16 *qkv_wp2 = nullptr;                              // qkv_wf in head-pair order (tld_refresh_math.h: qkv_pair_row; the two-head form of that kernel, EPI_QKV_ATTN2)
    float *qkv_c1p2 = nullptr, *qkv_b1p2 = nullptr;       // the same permutation of qkv_c1 / qkv_b1
    float *up_b = nullptr, *dw_w9c = nullptr, *dw_b = nullptr, *down_b = nullptr;
    float *dw_w9c_half = nullptr, *dw_b_half = nullptr;   // 0.5 x (exact): operands of the fused up-projection epilogue
    uint32_t* dw_wpk = nullptr;                           // the halved taps as packed bf16 pairs [3][4][hid] (EPI_UP_DWCONV2)
    // MX-fp8 GEMM mode (tld_engine_set_gemm_dtype): e4m3 weights + E8M0 block scales [K/128][N][4]
    uint8_t *qkv_w8 = nullptr, *qkv_s8 = nullptr, *up_w8 = nullptr, *up_s8 = nullptr, *down_w8 = nullptr, *down_s8 = nullptr;
    bf16 *up_wf = nullptr;                                // bf16(gamma3 (.) Wup): LayerNorm-3 folded into the up-projection
    float *up_c1 = nullptr, *up_b1 = nullptr;             // [hid] column sums of up_wf; up_b + beta3 . Wup^T
    float *n1_w = nullptr, *n1_b = nullptr, *n2_w = nullptr, *n2_b = nullptr, *n3_w = nullptr, *n3_b = nullptr;
    float *kv_w = nullptr, *q_w = nullptr;   // fp32, conditioning path
};

// The table finalize allocates from and the stage hook names from: the member of Layer (its name and offset), the "img.<name>" stage behind "blk<i>." (null: the image is read under an
// operand name instead -- wqkv / wup / wdown and their side tables -- or under none), element type and shape, elements allocated beyond the image (no weight), and
// whether this plan holds it.  Only the copies the engine's paths read are resident: the LayerNorm folds use gamma-scaled copies, the fp8 mode its own e4m3 ones.
struct BodyImage {
    const char* id; size_t member; const char* name; int dtype; int64_t shape[4]; int64_t margin; bool held;
    int64_t numel() const { return shape[0] * shape[1] * shape[2] * shape[3]; }
    void* get(const Layer& ly) const { void* p; memcpy(&p, reinterpret_cast<const char*>(&ly) + member, sizeof p); return p; }
    void set(Layer& ly, void* p) const { memcpy(reinterpret_cast<char*>(&ly) + member, &p, sizeof p); }
};
inline std::vector<BodyImage> body_block_images(const BodyShape& s, const BodyPlan& p) {
    const int64_t d = s.d, hid = s.hid;
    const bool bf = !p.fp8, f1 = p.fold_ln1, qa = p.fused_qa, pr = p.pair_held, f8 = p.fp8;
#define TLD_BI(m, name, dt, s0, s1, s2, s3, margin, held) BodyImage{#m, offsetof(Layer, m), name, dt, {s0, s1, s2, s3}, margin, held}
    return {
        TLD_BI(qkv_w, nullptr, ST_BF16, 3 * d, d, 1, 1, 0, bf && !f1), TLD_BI(up_w, nullptr, ST_BF16, hid, d, 1, 1, 0, bf && !p.fold_ln3), TLD_BI(down_w, nullptr, ST_BF16, d, hid, 1, 1, 0, bf),
        TLD_BI(kv_w, "kv_w", ST_F32, 2 * d, d, 1, 1, 0, true), TLD_BI(q_w, "q_w", ST_F32, d, d, 1, 1, 0, true), TLD_BI(up_b, "up_b", ST_F32, hid, 1, 1, 1, 0, true),
        TLD_BI(dw_b, "dw_b", ST_F32, hid, 1, 1, 1, 0, true), TLD_BI(down_b, "down_b", ST_F32, d, 1, 1, 1, 0, true), TLD_BI(n1_w, "n1_w", ST_F32, d, 1, 1, 1, 0, true),
        TLD_BI(n1_b, "n1_b", ST_F32, d, 1, 1, 1, 0, true), TLD_BI(n2_w, "n2_w", ST_F32, d, 1, 1, 1, 0, true), TLD_BI(n2_b, "n2_b", ST_F32, d, 1, 1, 1, 0, true),
        TLD_BI(n3_w, "n3_w", ST_F32, d, 1, 1, 1, 0, true), TLD_BI(n3_b, "n3_b", ST_F32, d, 1, 1, 1, 0, true),
        TLD_BI(qkv_wf, "qkv_wf", ST_BF16, 3 * d, d, 1, 1, 0, f1), TLD_BI(qkv_c1, "qkv_c1", ST_F32, 3 * d, 1, 1, 1, 0, f1), TLD_BI(qkv_b1, "qkv_b1", ST_F32, 3 * d, 1, 1, 1, 0, f1),
        // rows [q; k; v] x [head][64]  ->  [head][feature half][q | k | v][32]: tile-column h of the fused kernel is head h, and each of its two 96-column wave columns holds
        // 32 features of q, of k AND of v -- so the slow part of the image write (V^T: 2-byte scattered LDS writes) is shared by all eight waves instead of falling on the
        // four that held v (the values and their accumulation order do not change).  (+64: the side-table DMA of the last head reads a 256-column window)
        TLD_BI(qkv_wp, "qkv_wp", ST_BF16, 3 * d, d, 1, 1, 0, qa), TLD_BI(qkv_c1p, "qkv_c1p", ST_F32, 3 * d, 1, 1, 1, 64, qa), TLD_BI(qkv_b1p, "qkv_b1p", ST_F32, 3 * d, 1, 1, 1, 64, qa),
        // the same rows in head-pair order (EPI_QKV_ATTN2): 3 d^2 bf16 more per block
        TLD_BI(qkv_wp2, nullptr, ST_BF16, 3 * d, d, 1, 1, 0, pr), TLD_BI(qkv_c1p2, nullptr, ST_F32, 3 * d, 1, 1, 1, 0, pr), TLD_BI(qkv_b1p2, nullptr, ST_F32, 3 * d, 1, 1, 1, 0, pr),
        TLD_BI(up_wf, nullptr, ST_BF16, hid, d, 1, 1, 0, p.fold_ln3), TLD_BI(up_c1, nullptr, ST_F32, hid, 1, 1, 1, 0, p.fold_ln3), TLD_BI(up_b1, nullptr, ST_F32, hid, 1, 1, 1, 0, p.fold_ln3),
        // depthwise taps [hid,1,3,3] -> [9][hid]; halved copies for the fused epilogue (its GELU is written for x / 2; scaling by 0.5 is exact); packed bf16 tap pairs for
        // the v_dot2c form
        TLD_BI(dw_w9c, "dw_w9c", ST_F32, 9, hid, 1, 1, 0, true), TLD_BI(dw_w9c_half, "dw_w9c_half", ST_F32, 9, hid, 1, 1, 0, true), TLD_BI(dw_b_half, "dw_b_half", ST_F32, hid, 1, 1, 1, 0, true),
        TLD_BI(dw_wpk, "dw_wpk", ST_BF16, 3, 4, hid, 2, 0, true),
        TLD_BI(qkv_w8, "qkv_w8", ST_U8, 3 * d, d, 1, 1, 0, f8), TLD_BI(qkv_s8, "qkv_s8", ST_MX8S, 3 * d, d / 32, 1, 1, 0, f8), TLD_BI(up_w8, "up_w8", ST_U8, hid, d, 1, 1, 0, f8),
        TLD_BI(up_s8, "up_s8", ST_MX8S, hid, d / 32, 1, 1, 0, f8), TLD_BI(down_w8, "down_w8", ST_U8, d, hid, 1, 1, 0, f8), TLD_BI(down_s8, "down_s8", ST_MX8S, d, hid / 32, 1, 1, 0, f8)};
#undef TLD_BI
}

// ---- the snapshots the stage hook reserves for a forward of max_batch samples: exactly the SNAP / sink names run_body and the samplers use under this plan -------------
// ONE exception, kept: a low-latency engine that holds the folded-tail image reserves the last block's "mlp" at 4 bytes per element although its row is a residual-stream
// snapshot.  `splitk_slices`: the slices of the split-K buffer the engine holds (it outlives its class).
struct BodyStage { std::string name; size_t bytes; };
inline std::vector<BodyStage> body_stages(const BodyShape& s, const BodyPlan& p, int max_batch, int splitk_slices) {
    const size_t B = (size_t)max_batch, M = B * s.ntok, d = s.d, hid = s.hid, rs = sizeof(resid_t);
    std::vector<BodyStage> v;
    v.push_back({"tokens0", M * d * rs});
    for (const char* n : {"out", "step.x_t", "step.x0_prev", "step.x0", "step.x_next", "step.out"}) v.push_back({n, B * s.img * 4});
    for (int l = 0; l < s.L; ++l) {
        const std::string b = "blk" + std::to_string(l) + ".";
        auto add = [&v, &b](const char* n, size_t bytes) { v.push_back({b + n, bytes}); };
        add("x_in", M * d * rs); add("ca", M * d * rs);
        add("mlp", M * d * ((l + 1 == s.L && p.fold_tail_held) ? 4 : rs));      // (the folded tail: the last block's row is an fp32 debug evaluation)
        add("att", M * d * 2); add("sa", M * d * 4);
        if (p.fold_ln1) add("ln1", M * kLnSlots * 8); else if (!p.ln_mx8) add("xn1", M * d * 2);
        if (!p.fused_qa) { add("qk", M * 2 * d * 2); add("vt", M * d * 2); }
        if (p.fold_ln3) add("stats", M * 8); else if (!p.cross_mx8) add("xn3", M * d * 2);
        if (!p.fuse_dw) add("hid_pre", M * hid * 2);
        if (p.fp8) {   // the three A operands as the GEMMs read them: e4m3 codes, and the E8M0 scales of the call's rows
            add("a8_qkv.q", M * d); add("a8_qkv.s", M * d / 32); add("a8_up.q", M * d); add("a8_up.s", M * d / 32);
            add("a8_down.q", M * hid); add("a8_down.s", M * hid / 32);
        }
        if (!p.dw_mx8) add("hid", M * hid * 2);      // (the quantising depthwise kernels write no bf16 copy)
        if (splitk_slices) add("splitk", (size_t)splitk_slices * M * d * 4);
    }
    return v;
}

}  // namespace tld

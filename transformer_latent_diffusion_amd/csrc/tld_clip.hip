// tld_clip.hip -- CLIP text tower on gfx950: the front edge of the pipeline.
//
// Replaces `model.encode_text(text_tokens)` of the reference's encode_text (tld/diffusion.py:136-140), where `model` is
// OpenAI CLIP "ViT-L/14" loaded by `clip.load` (tld/diffusion.py:160, tld/configs.py:46-48) -- a third-party package that is
// not part of the reference checkout.  What is restated is CLIP.encode_text of openai/CLIP (clip/model.py):
//   x = token_embedding[text] + positional_embedding
//   12 x ResidualAttentionBlock: x += MHA(ln_1(x), causal mask);  x += c_proj(QuickGELU(c_fc(ln_2(x))))
//   x = ln_final(x);  out = x[arange(B), text.argmax(-1)] @ text_projection
// Tokenisation (a Python BPE over a vocabulary file) stays on the host; this engine takes token ids.
//
// Layout: the residual stream is fp32 [B*ctx, width]; LayerNorm outputs and the projections' operands are bf16; the four
// projections of a block are the persistent MFMA GEMM of tld_gemm.hip (bias -> bf16, or fp32 out for the two that end in the
// residual add); the add, its bias and the next LayerNorm are one row kernel; causal attention over <= 128 tokens with
// head_dim 64 is a one-wave-per-(sample, head) fp32 kernel (77 x 77 scores: no tile to speak of).  One prompt batch is
// ~13 GFLOP per prompt: this path is about removing the host round trip, not about its own speed.
#include "../../include/tld_hip.h"
#include "tld_common.h"
#include "tld_host.h"
#include "tld_clip_kernels.h"      // clip_add_ln_kernel, clip_final_ln_kernel, clip_quickgelu_kernel, gemm: shared with tld_clip_vision.hip
#include "tld_clip_core.h"         // ClipCore: the engine's state, weights, stage hook and block runner, shared with tld_clip_vision.hip

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace tld;

namespace {

// ---- kernels -----------------------------------------------------------------------------------------------------------

// x[t] = token_embedding[text[t]] + positional_embedding[t % ctx]      (clip/model.py encode_text, first two lines)
__global__ void clip_embed_kernel(const int* __restrict__ tokens, const float* __restrict__ tok_emb, const float* __restrict__ pos,
                                  float* __restrict__ x, int T, int W, int ctx, int vocab) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)T * W) return;
    const int t = (int)(i / W), c = (int)(i - (long)t * W);
    int id = tokens[t];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    x[i] = tok_emb[(size_t)id * W + c] + pos[(size_t)(t % ctx) * W + c];
}

// Causal multi-head attention, head_dim 64, ctx <= 128 tokens: one wave per (head, sample).  q | k | v are the bf16 rows of the
// in_proj GEMM ([T, 3W]: q at column h*64, k at W + h*64, v at 2W + h*64 -- nn.MultiheadAttention's packed in_proj order).
//   scores s_ij = q_i . k_j / 8 for j <= i (attn_mask: -inf above the diagonal), softmax over j, o_i = sum_j p_ij v_j.
// Lane j owns keys j and j + 64 in the score phase and output feature j in the value phase.
__global__ __launch_bounds__(64) void clip_attn_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out, int ctx, int W) {
    extern __shared__ float sm[];
    float* Qs = sm;                        // [ctx][64]
    float* Ks = Qs + ctx * 64;             // [ctx][65]  (pitch 65: lane j reads row j)
    float* Vs = Ks + ctx * 65;             // [ctx][64]
    float* P = Vs + ctx * 64;              // [128]
    const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const bf16* base = qkv + (size_t)b * ctx * 3 * W + h * 64;
    for (int i = 0; i < ctx; ++i) {
        const bf16* r = base + (size_t)i * 3 * W;
        Qs[i * 64 + lane] = (float)r[lane];
        Ks[i * 65 + lane] = (float)r[W + lane];
        Vs[i * 64 + lane] = (float)r[2 * W + lane];
    }
    __syncthreads();
    const int j0 = lane, j1 = lane + 64;
    for (int i = 0; i < ctx; ++i) {
        float s0 = -INFINITY, s1 = -INFINITY;
        if (j0 <= i) {
            float a = 0.f;
            for (int k = 0; k < 64; ++k) a = fmaf(Qs[i * 64 + k], Ks[j0 * 65 + k], a);
            s0 = a * 0.125f;
        }
        if (j1 <= i) {                     // (j1 <= i < ctx)
            float a = 0.f;
            for (int k = 0; k < 64; ++k) a = fmaf(Qs[i * 64 + k], Ks[j1 * 65 + k], a);
            s1 = a * 0.125f;
        }
        float m = fmaxf(s0, s1);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const float e0 = j0 <= i ? expf(s0 - m) : 0.f, e1 = j1 <= i ? expf(s1 - m) : 0.f;
        const float inv = 1.0f / wave_sum(e0 + e1);
        P[j0] = e0 * inv; P[j1] = e1 * inv;
        __syncthreads();
        float o = 0.f;
        for (int j = 0; j <= i; ++j) o = fmaf(P[j], Vs[j * 64 + lane], o);
        out[((size_t)b * ctx + i) * W + h * 64 + lane] = (bf16)o;
        __syncthreads();
    }
}

}  // namespace

struct tld_clip : ClipCore {                  // the transformer, its workspace and the stage hook: tld_clip_core.h
    int ctx = 0, V = 0;
    float *tok_emb = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr;
};

extern "C" {

int tld_clip_create(const tld_clip_config* cfg, tld_clip** out) {
    if (!cfg || !out) return fail(TLD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_transformer(cfg->width, cfg->heads, cfg->layers)) return rc;
    if (cfg->context_length < 1 || cfg->context_length > 128) return fail(TLD_ERR_INVALID, "context_length=%d: 1..128", cfg->context_length);
    if (cfg->embed_dim < 1 || cfg->vocab_size < 1 || cfg->max_batch < 1) return fail(TLD_ERR_INVALID, "embed_dim / vocab_size / max_batch must be positive");
    if (const std::string bad = clip_reach_check(cfg->max_batch, cfg->context_length, cfg->width); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    if (int rc = check_device(cfg->device_id, "text")) return rc;
    DeviceGuard guard(cfg->device_id);
    tld_clip* c = new tld_clip();
    c->W = cfg->width; c->L = cfg->layers; c->H = cfg->heads; c->E = cfg->embed_dim; c->max_batch = cfg->max_batch; c->device_id = cfg->device_id;
    c->ctx = cfg->context_length; c->V = cfg->vocab_size;
    if (int rc = alloc_workspace(c, c->ctx)) { tld_clip_destroy(c); return rc; }
    *out = c;
    return TLD_OK;
}

int tld_clip_load_tensor(tld_clip* c, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
    return load_tensor(c, CLIP_TEXT, key, host_ptr, shape, ndim, dtype);
}

int tld_clip_finalize_weights(tld_clip* c) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    if (c->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    DeviceGuard guard(c->device_id);
    const int W = c->W;
    if (int rc = upload_entry(c, "token_embedding.weight", {c->V, W}, &c->tok_emb)) return rc;
    if (int rc = upload_entry(c, "positional_embedding", {c->ctx, W}, &c->pos)) return rc;
    if (int rc = upload_entry(c, "ln_final.weight", {W}, &c->lnf_g)) return rc;
    if (int rc = upload_entry(c, "ln_final.bias", {W}, &c->lnf_b)) return rc;
    if (int rc = upload_proj_t(c, "text_projection")) return rc;
    if (int rc = upload_blocks(c, CLIP_TEXT)) return rc;
    return finish_weights(c);
}

int tld_clip_encode_text(tld_clip* c, const int32_t* tokens, const int32_t* eot_index, float* out, int32_t batch, void* hip_stream) {
    if (!c || !tokens || !eot_index || !out) return fail(TLD_ERR_INVALID, "null argument");
    if (int rc = check_encode(c, batch)) return rc;
    DeviceGuard guard(c->device_id);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int W = c->W, ctx = c->ctx, T = batch * ctx;
    if (c->debug) { if (int rc = begin_debug_call(c, ctx, "tld_clip_set_debug", s)) return rc; }
    {
        const long n = (long)T * W;
        hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tokens, c->tok_emb, c->pos, c->x, T, W, ctx, c->V);
    }
    const size_t attn_lds = (size_t)(ctx * 64 * 2 + ctx * 65 + 128) * sizeof(float);
    static PerDeviceOnce attr_set;
    attr_set.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(clip_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * (64 * 2 + 65) * 4 + 512); });
    auto attention = [&] { hipLaunchKernelGGL(clip_attn_kernel, dim3(c->H, batch), dim3(64), attn_lds, s, c->qkv, c->att, ctx, W); };
    if (int rc = run_blocks(c, batch, ctx, attention, eot_index, c->lnf_g, c->lnf_b, "tld_clip_encode_text", out, s)) return rc;
    return check_launch("encode_text");
}

int tld_clip_set_debug(tld_clip* c, int32_t enable) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    DeviceGuard guard(c->device_id);
    if (!enable) { drop_snapshots(c); return TLD_OK; }
    if (c->debug) return TLD_OK;
    if (reserve_stages(c, c->ctx)) {
        drop_snapshots(c);
        return fail(TLD_ERR_HIP, "tld_clip_set_debug: no memory for the stage snapshots of %d prompts x %d layers; debug stays off", c->max_batch, c->L);
    }
    c->debug = true;
    return TLD_OK;
}

int tld_clip_read_stage(tld_clip* c, const char* name, float* host_out, int64_t numel, int64_t* shape4) { return read_stage(c, name, host_out, numel, shape4); }

int64_t tld_clip_weight_bytes(const tld_clip* c) { return weight_bytes(c); }

int tld_clip_destroy(tld_clip* c) {
    if (!c) return TLD_OK;
    release(c);
    delete c;
    return TLD_OK;
}

}  // extern "C"

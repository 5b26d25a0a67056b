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

struct Block {
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    bf16 *in_w = nullptr, *out_w = nullptr, *fc_w = nullptr, *proj_w = nullptr;
    float *in_b = nullptr, *out_b = nullptr, *fc_b = nullptr, *proj_b = nullptr;
};

}  // namespace

struct tld_clip : DeviceArena {
    tld_clip_config cfg{};
    int W = 0, L = 0, H = 0, ctx = 0, E = 0, V = 0;
    bool finalized = false;
    std::map<std::string, HostTensor> host;
    float *tok_emb = nullptr, *pos = nullptr, *lnf_g = nullptr, *lnf_b = nullptr, *proj_t = nullptr;     // proj_t: text_projection^T [E][W]
    std::vector<Block> blocks;
    // workspace (max_batch * ctx rows)
    float *x = nullptr, *tmp = nullptr, *pooled = nullptr;
    bf16 *h = nullptr, *qkv = nullptr, *att = nullptr, *f = nullptr;
    // stage capture (tld_clip_set_debug): snapshot memory for max_batch prompts, allocated by set_debug(1), freed by set_debug(0) / destroy
    bool debug = false;
    StageStore stages;                        // the stage hook (tld_host.h); the operands are named in it from finalize_weights on
};

namespace {

int need(const tld_clip* c, const std::string& key, const std::vector<int64_t>& shape, const HostTensor** out) {
    auto it = c->host.find(key);
    if (it == c->host.end()) return fail(TLD_ERR_STATE, "missing state_dict entry '%s'", key.c_str());
    if (it->second.shape != shape) {
        std::string got, want;
        for (int64_t s : it->second.shape) got += std::to_string(s) + ",";
        for (int64_t s : shape) want += std::to_string(s) + ",";
        return fail(TLD_ERR_SHAPE, "'%s' has shape [%s], expected [%s]", key.c_str(), got.c_str(), want.c_str());
    }
    *out = &it->second;
    return TLD_OK;
}
// the GEMM operands as the engine holds them, logical [N][K], read in place: named once the weights exist, whether or not the hook is on
void name_operands(tld_clip* c) {
    const int64_t W = c->W;
    c->stages.ref("proj_t", c->proj_t, ST_F32, c->E, W);
    for (int l = 0; l < (int)c->blocks.size(); ++l) {
        const Block& b = c->blocks[l];
        const std::string pre = "blk" + std::to_string(l) + ".";
        c->stages.ref(pre + "in_w", b.in_w, ST_BF16, 3 * W, W); c->stages.ref(pre + "out_w", b.out_w, ST_BF16, W, W);
        c->stages.ref(pre + "fc_w", b.fc_w, ST_BF16, 4 * W, W); c->stages.ref(pre + "proj_w", b.proj_w, ST_BF16, W, 4 * W);
    }
}
// set_debug(0) / destroy: the snapshots go, the operand names stay
void drop_snapshots(tld_clip* c) {
    c->stages.free_all();
    c->debug = false;
    if (c->finalized) name_operands(c);
}

}  // namespace

extern "C" {

int tld_clip_create(const tld_clip_config* cfg, tld_clip** out) {
    if (!cfg || !out) return fail(TLD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->width < 64 || cfg->width > 1024 || cfg->width % 64) return fail(TLD_ERR_INVALID, "width=%d: a multiple of 64 in 64..1024", cfg->width);
    if (cfg->heads * 64 != cfg->width) return fail(TLD_ERR_INVALID, "heads=%d: head_dim must be 64 (width / heads)", cfg->heads);
    if (cfg->layers < 1 || cfg->layers > 64) return fail(TLD_ERR_INVALID, "layers=%d: 1..64", cfg->layers);
    if (cfg->context_length < 1 || cfg->context_length > 128) return fail(TLD_ERR_INVALID, "context_length=%d: 1..128", cfg->context_length);
    if (cfg->embed_dim < 1 || cfg->vocab_size < 1 || cfg->max_batch < 1) return fail(TLD_ERR_INVALID, "embed_dim / vocab_size / max_batch must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TLD_ERR_HIP, "no HIP device available (the text tower has no CPU path)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(TLD_ERR_INVALID, "device_id=%d out of range (%d devices)", cfg->device_id, ndev);
    DeviceGuard guard(cfg->device_id);
    tld_clip* c = new tld_clip();
    c->cfg = *cfg;
    c->W = cfg->width; c->L = cfg->layers; c->H = cfg->heads; c->ctx = cfg->context_length; c->E = cfg->embed_dim; c->V = cfg->vocab_size;
    const size_t T = (size_t)cfg->max_batch * c->ctx, W = c->W;
    auto bail = [&](int rc) { tld_clip_destroy(c); return rc; };
    if (int rc = dev_alloc(c, &c->x, T * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->tmp, T * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->pooled, (size_t)cfg->max_batch * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->h, T * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->qkv, T * 3 * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->att, T * W)) return bail(rc);
    if (int rc = dev_alloc(c, &c->f, T * 4 * W)) return bail(rc);
    *out = c;
    return TLD_OK;
}

int tld_clip_load_tensor(tld_clip* c, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
    if (!c || !key || (!host_ptr && ndim > 0) || ndim < 0 || ndim > 8) return fail(TLD_ERR_INVALID, "bad argument");
    if (c->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    std::string k(key);
    if (k.rfind("visual.", 0) == 0 || k == "logit_scale" || k == "input_resolution" || k == "context_length" || k == "vocab_size")
        return TLD_OK;                                      // the image tower and the archive's metadata are not used by encode_text
    const bool known = k == "token_embedding.weight" || k == "positional_embedding" || k == "text_projection" ||
                       k.rfind("ln_final.", 0) == 0 || k.rfind("transformer.resblocks.", 0) == 0;
    if (!known) return fail(TLD_ERR_KEY, "unknown state_dict key '%s'", key);
    if (dtype != TLD_DTYPE_F32) return fail(TLD_ERR_INVALID, "'%s': host tensors must be fp32", key);
    HostTensor t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { if (shape[i] < 0) return fail(TLD_ERR_SHAPE, "'%s': negative dimension", key); t.shape.push_back(shape[i]); n *= shape[i]; }
    t.data.assign(reinterpret_cast<const float*>(host_ptr), reinterpret_cast<const float*>(host_ptr) + n);
    c->host[k] = std::move(t);
    return TLD_OK;
}

int tld_clip_finalize_weights(tld_clip* c) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    if (c->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    DeviceGuard guard(c->cfg.device_id);
    const int W = c->W, E = c->E;
    const HostTensor* t = nullptr;
    if (int rc = need(c, "token_embedding.weight", {c->V, W}, &t)) return rc;
    if (int rc = upload_f32(c, t->data, &c->tok_emb)) return rc;
    if (int rc = need(c, "positional_embedding", {c->ctx, W}, &t)) return rc;
    if (int rc = upload_f32(c, t->data, &c->pos)) return rc;
    if (int rc = need(c, "ln_final.weight", {W}, &t)) return rc;
    if (int rc = upload_f32(c, t->data, &c->lnf_g)) return rc;
    if (int rc = need(c, "ln_final.bias", {W}, &t)) return rc;
    if (int rc = upload_f32(c, t->data, &c->lnf_b)) return rc;
    if (int rc = need(c, "text_projection", {W, E}, &t)) return rc;
    {
        std::vector<float> pt((size_t)E * W);
        for (int k = 0; k < W; ++k) for (int n = 0; n < E; ++n) pt[(size_t)n * W + k] = t->data[(size_t)k * E + n];
        if (int rc = upload_f32(c, pt, &c->proj_t)) return rc;
    }
    c->blocks.resize(c->L);
    for (int l = 0; l < c->L; ++l) {
        Block& b = c->blocks[l];
        const std::string p = "transformer.resblocks." + std::to_string(l) + ".";
        struct Item { const char* key; std::vector<int64_t> shape; float** f32; bf16** b16; };
        const std::vector<Item> items = {
            {"ln_1.weight", {W}, &b.ln1_g, nullptr}, {"ln_1.bias", {W}, &b.ln1_b, nullptr},
            {"attn.in_proj_weight", {3 * W, W}, nullptr, &b.in_w}, {"attn.in_proj_bias", {3 * W}, &b.in_b, nullptr},
            {"attn.out_proj.weight", {W, W}, nullptr, &b.out_w}, {"attn.out_proj.bias", {W}, &b.out_b, nullptr},
            {"ln_2.weight", {W}, &b.ln2_g, nullptr}, {"ln_2.bias", {W}, &b.ln2_b, nullptr},
            {"mlp.c_fc.weight", {4 * W, W}, nullptr, &b.fc_w}, {"mlp.c_fc.bias", {4 * W}, &b.fc_b, nullptr},
            {"mlp.c_proj.weight", {W, 4 * W}, nullptr, &b.proj_w}, {"mlp.c_proj.bias", {W}, &b.proj_b, nullptr},
        };
        for (auto& it : items) {
            if (int rc = need(c, p + it.key, it.shape, &t)) return rc;
            if (it.f32) { if (int rc = upload_f32(c, t->data, it.f32)) return rc; }
            else { if (int rc = upload_bf16(c, t->data, it.b16)) return rc; }
        }
    }
    c->host.clear();
    HIP_TRY(hipDeviceSynchronize());
    c->finalized = true;
    name_operands(c);
    return TLD_OK;
}

int tld_clip_encode_text(tld_clip* c, const int32_t* tokens, const int32_t* eot_index, float* out, int32_t batch, void* hip_stream) {
    if (!c || !tokens || !eot_index || !out) return fail(TLD_ERR_INVALID, "null argument");
    if (!c->finalized) return fail(TLD_ERR_STATE, "weights not finalized");
    if (batch < 1 || batch > c->cfg.max_batch) return fail(TLD_ERR_INVALID, "batch=%d outside 1..max_batch=%d", batch, c->cfg.max_batch);
    DeviceGuard guard(c->cfg.device_id);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int W = c->W, ctx = c->ctx, T = batch * ctx;
    const bool dbg = c->debug;
    if (dbg) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
            return fail(TLD_ERR_STATE, "a debug encode (tld_clip_set_debug) cannot be captured into a graph");
        c->stages.begin_call();
        const size_t TW = (size_t)c->cfg.max_batch * ctx * W;        // the whole workspace: NaN in bf16 and fp32 wherever this call stores nothing
        HIP_TRY(hipMemsetAsync(c->x, 0xFF, TW * 4, s));
        HIP_TRY(hipMemsetAsync(c->tmp, 0xFF, TW * 4, s));
        HIP_TRY(hipMemsetAsync(c->pooled, 0xFF, (size_t)c->cfg.max_batch * W * 4, s));
        HIP_TRY(hipMemsetAsync(c->h, 0xFF, TW * 2, s));
        HIP_TRY(hipMemsetAsync(c->qkv, 0xFF, TW * 3 * 2, s));
        HIP_TRY(hipMemsetAsync(c->att, 0xFF, TW * 2, s));
        HIP_TRY(hipMemsetAsync(c->f, 0xFF, TW * 4 * 2, s));
    }
#define KEEP(name, src, dtype, rows, cols) do { if (dbg) { if (int rc_ = c->stages.copy(name, src, dtype, s, rows, cols)) return rc_; } } while (0)
#define GEMM(what, ...) GEMM_TRY("tld_clip_encode_text, block " + std::to_string(l) + " " what, gemm(__VA_ARGS__))
    {
        const long n = (long)T * W;
        hipLaunchKernelGGL(clip_embed_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tokens, c->tok_emb, c->pos, c->x, T, W, ctx, c->V);
    }
    const dim3 rows((T + 3) / 4);
    const size_t attn_lds = (size_t)(ctx * 64 * 2 + ctx * 65 + 128) * sizeof(float);
    static PerDeviceOnce attr_set;
    attr_set.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(clip_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * (64 * 2 + 65) * 4 + 512); });
    KEEP("x0", c->x, ST_F32, T, W);
    hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, (const float*)nullptr, (const float*)nullptr, c->blocks[0].ln1_g, c->blocks[0].ln1_b, c->h, T, W);
    for (int l = 0; l < c->L; ++l) {
        const Block& b = c->blocks[l];
        const std::string pre = dbg ? "blk" + std::to_string(l) + "." : std::string();
        KEEP(pre + "h1", c->h, ST_BF16, T, W);
        GEMM("in_proj", c->h, W, b.in_w, T, 3 * W, W, EPI_BIAS_BF16, b.in_b, c->qkv, nullptr, s);
        KEEP(pre + "qkv", c->qkv, ST_BF16, T, 3 * W);
        hipLaunchKernelGGL(clip_attn_kernel, dim3(c->H, batch), dim3(64), attn_lds, s, c->qkv, c->att, ctx, W);
        KEEP(pre + "att", c->att, ST_BF16, T, W);
        GEMM("out_proj", c->att, W, b.out_w, T, W, W, EPI_F32, nullptr, nullptr, c->tmp, s);
        KEEP(pre + "attn_out", c->tmp, ST_F32, T, W);
        hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, c->tmp, b.out_b, b.ln2_g, b.ln2_b, c->h, T, W);
        KEEP(pre + "x1", c->x, ST_F32, T, W);
        KEEP(pre + "h2", c->h, ST_BF16, T, W);
        GEMM("c_fc", c->h, W, b.fc_w, T, 4 * W, W, EPI_BIAS_BF16, b.fc_b, c->f, nullptr, s);
        KEEP(pre + "f_pre", c->f, ST_BF16, T, 4 * W);
        {
            const long n8 = (long)T * 4 * W / 8;
            hipLaunchKernelGGL(clip_quickgelu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, c->f, n8);
        }
        KEEP(pre + "f", c->f, ST_BF16, T, 4 * W);
        GEMM("c_proj", c->f, 4 * W, b.proj_w, T, W, 4 * W, EPI_F32, nullptr, nullptr, c->tmp, s);
        KEEP(pre + "mlp_out", c->tmp, ST_F32, T, W);
        if (l + 1 < c->L) {
            hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, c->tmp, b.proj_b, c->blocks[l + 1].ln1_g, c->blocks[l + 1].ln1_b, c->h, T, W);
            KEEP(pre + "x2", c->x, ST_F32, T, W);
        } else {
            hipLaunchKernelGGL(clip_final_ln_kernel, dim3(batch), dim3(64), 0, s, c->x, c->tmp, b.proj_b, eot_index, c->lnf_g, c->lnf_b, c->pooled, W, ctx);
            KEEP("pooled", c->pooled, ST_F32, batch, W);
        }
    }
    launch_linear_f32(c->pooled, W, c->proj_t, nullptr, out, c->E, batch, W, c->E, 0, s);
    KEEP("out", out, ST_F32, batch, c->E);
#undef KEEP
#undef GEMM
    return check_launch("encode_text");
}

int tld_clip_set_debug(tld_clip* c, int32_t enable) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    DeviceGuard guard(c->cfg.device_id);
    if (!enable) { drop_snapshots(c); return TLD_OK; }
    if (c->debug) return TLD_OK;
    // memory for every stage of max_batch prompts: T rows per block stage, one row per prompt for the pooled row and the output
    const size_t B = (size_t)c->cfg.max_batch, T = B * c->ctx, W = c->W;
    int rc = c->stages.reserve("x0", T * W * 4);
    for (int l = 0; !rc && l < c->L; ++l) {
        const std::string pre = "blk" + std::to_string(l) + ".";
        for (const char* n : {"h1", "att", "h2"}) if (!rc) rc = c->stages.reserve(pre + n, T * W * 2);
        for (const char* n : {"attn_out", "x1", "mlp_out"}) if (!rc) rc = c->stages.reserve(pre + n, T * W * 4);
        if (!rc) rc = c->stages.reserve(pre + "qkv", T * 3 * W * 2);
        for (const char* n : {"f_pre", "f"}) if (!rc) rc = c->stages.reserve(pre + n, T * 4 * W * 2);
        if (!rc && l + 1 < c->L) rc = c->stages.reserve(pre + "x2", T * W * 4);              // the last block forms only the pooled rows
    }
    if (!rc) rc = c->stages.reserve("pooled", B * W * 4);
    if (!rc) rc = c->stages.reserve("out", B * c->E * 4);
    if (rc) {
        drop_snapshots(c);
        return fail(TLD_ERR_HIP, "tld_clip_set_debug: no memory for the stage snapshots of %d prompts x %d layers; debug stays off", c->cfg.max_batch, c->L);
    }
    c->debug = true;
    return TLD_OK;
}

int tld_clip_read_stage(tld_clip* c, const char* name, float* host_out, int64_t numel, int64_t* shape4) {
    if (!c || !name || !host_out) return fail(TLD_ERR_INVALID, "null argument");
    DeviceGuard guard(c->cfg.device_id);
    return c->stages.read(name, host_out, numel, shape4);
}

int64_t tld_clip_weight_bytes(const tld_clip* c) { return c ? c->weight_bytes : 0; }

int tld_clip_destroy(tld_clip* c) {
    if (!c) return TLD_OK;
    DeviceGuard guard(c->cfg.device_id);
    drop_snapshots(c);
    for (void* p : c->allocs) (void)hipFree(p);
    delete c;
    return TLD_OK;
}

}  // extern "C"

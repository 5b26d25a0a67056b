// tld_clip_vision.hip -- CLIP image tower on gfx950: image embeddings in the joint space the denoiser's labels live in.
//
// Restates VisionTransformer.forward of openai/CLIP (clip/model.py), which `model.encode_image(preprocess(img))` runs:
//   x = conv1(pixels)                      # patch x patch, stride patch, no bias -> [B, g*g, W]
//   x = cat(class_embedding, x) + positional_embedding        # [B, n = g*g + 1, W]
//   x = ln_pre(x)
//   L x ResidualAttentionBlock (no mask): x += MHA(ln_1(x));  x += c_proj(QuickGELU(c_fc(ln_2(x))))
//   out = ln_post(x[:, 0]) @ proj          # [B, embed_dim]
//
// Layout: as the text tower (tld_clip.hip) -- fp32 residual stream [B*n, W], bf16 LayerNorm outputs and GEMM operands, the projections on the
// persistent MFMA GEMM of tld_gemm.hip, the add + LayerNorm row kernels and QuickGELU shared with it (tld_clip_kernels.h).  The patch embedding
// is an im2col into bf16 rows [B*g*g, Kp] (3 p*p zero-padded to a multiple of 64) and the same GEMM.  What is new is attention: non-causal,
// n = g*g + 1 tokens (never a multiple of a tile), on MFMA -- clip_vis_attn_kernel below.
#include "../../include/tld_hip.h"
#include "tld_common.h"
#include "tld_host.h"
#include "tld_clip_kernels.h"      // clip_add_ln_kernel, clip_final_ln_kernel, clip_quickgelu_kernel, gemm: shared with tld_clip.hip
#include "tld_clip_core.h"         // ClipCore: the engine's state, weights, stage hook and block runner, shared with tld_clip.hip

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace tld;

namespace {

constexpr int kMaxGrid = 16;                      // g <= 16: n <= 257 tokens
constexpr int kMaxKeyTiles = (kMaxGrid * kMaxGrid + 1 + 31) / 32;      // 9 tiles of 32 keys
constexpr int kKPitch = 72;                       // bf16 per K row in LDS: 64 + 8 (144 B: 16-byte aligned rows, consecutive rows 4 banks apart)

// pitch of one feature row of the transposed V image, in bf16: >= keys, and (pitch / 2) % 32 == 2 so that the 32 lanes of a half-wave, which read
// 8 bytes each from 32 consecutive feature rows, fall on 32 distinct bank pairs
inline int v_pitch(int keys) {
    int p = keys;
    while ((p / 2) % 32 != 2 || p % 4) p += 2;
    return p;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------

// im2col of conv1 (kernel = stride = p, no padding): row (b, gy, gx), column k = (c * p + py) * p + px -- conv1.weight's own [3, p, p] order --
// = bf16(pixels[b, c, gy p + py, gx p + px]); columns 3 p*p .. Kp are zero.
template <typename T>
__global__ void clip_vis_im2col_kernel(const T* __restrict__ pix, bf16* __restrict__ rows, long total, int g, int p, int Kp) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int k = (int)(i % Kp);
    const long r = i / Kp;
    float v = 0.f;
    if (k < 3 * p * p) {
        const int gx = (int)(r % g), gy = (int)((r / g) % g);
        const long b = r / ((long)g * g);
        const int px = k % p, py = (k / p) % p, c = k / (p * p);
        const int R = g * p;
        v = (float)pix[((b * 3 + c) * R + (gy * p + py)) * (long)R + gx * p + px];
    }
    rows[i] = (bf16)v;
}

// One wave per token row:  x[row] = ln_pre((tok == 0 ? class_embedding : emb[b, tok - 1]) + positional_embedding[tok]), fp32 (the residual stream's start).
__global__ __launch_bounds__(256) void clip_vis_embed_ln_kernel(const float* __restrict__ emb, const float* __restrict__ cls, const float* __restrict__ pos,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ x,
                                                                int T, int W, int n) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    const int b = row / n, tok = row - b * n;
    const float* src = tok == 0 ? cls : emb + ((size_t)b * (n - 1) + (tok - 1)) * W;
    float v[16];
    const int m = W / 64;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < m) { const int c = j * 64 + lane; v[j] = src[c] + pos[(size_t)tok * W + c]; s += v[j]; }
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < m) { const float c = v[j] - mean; q = fmaf(c, c, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + kLnEps);
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < m) { const int c = j * 64 + lane; x[(size_t)row * W + c] = (v[j] - mean) * rstd * gamma[c] + beta[c]; }
}

// Non-causal multi-head attention on MFMA, head_dim 64, n tokens per sample with 2 <= n <= 257 arbitrary (n = g*g + 1 is never a multiple of the
// 32-token tile).  One workgroup of four waves per (head, sample); qkv is the in_proj GEMM's bf16 [T, 3W] rows (q at column h*64, k at W + h*64,
// v at 2W + h*64), out is bf16 [T, W].
//
// Structure.  NT = ceil(n / 32) key tiles.  The workgroup stages K as [NT*32][64] (pitch 72) and V TRANSPOSED as [64][NT*32] (pitch v_pitch) in LDS.
// Each wave then takes 32-query tiles qt = wave, wave + 4, ...:
//   S^T tile t = K_t . Q^T  (mfma 32x32x16 bf16, A = K rows from LDS, B = Q rows straight from global memory): the accumulator has the QUERY on the
//   lane (lane & 31) and the tile's 32 KEYS in its 16 registers x 2 lane halves -- key = 32 t + (i & 3) + 8 (i >> 2) + 4 (lane >> 5) for register i.
//   All NT tiles of scores stay in registers (at most 9 x 16), so the softmax is single-pass: row maximum and row sum are a reduction over a lane's
//   own registers and ONE exchange with lane ^ 32.
//   O^T = V^T . P^T: the score accumulator, converted to bf16, IS the B operand of the second product (it sums over the accumulator's row index:
//   no lane movement, no LDS); the A operand is V^T from LDS in the matching permuted key order (element j of lane half h of k-step s is key
//   32 t + 16 s + 8 (j >> 2) + 4 h + (j & 3): two 8-byte reads).  The result has the query on the lane and 4 consecutive features per register quad.
//
// Roundings (tests/clip_vision_refs.py attention_model restates them): q, k, v are the bf16 values as stored; scores accumulate in fp32 on the MFMA
// and are scaled by 1/8 (exact) in fp32; maximum, e = exp(s - max) and the row sum l = sum e are fp32 (the sum is over the UNROUNDED e); e is rounded
// to bf16 (RNE) as the operand of the PV product, which accumulates in fp32; o = acc / l in fp32, rounded to bf16 (RNE) on the store.
//
// The ragged end, by construction:
//   * keys >= n: their score is replaced by -inf BEFORE the maximum is taken and their e is the constant 0, not exp of anything: they weigh exactly 0
//     and cannot move the maximum, whatever the staged K row holds.
//   * K and V rows >= n are staged as zeros (a select on the loaded value), so a V row >= n contributes 0 x 0 even if memory there holds NaN.
//   * query rows >= n compute on a clamped copy of row n - 1 and are not stored (`q < n` guards the store).
//   * NO ADDRESS PAST THE SAMPLE'S LAST ROW IS FORMED: every global load -- K / V staging and the Q fragments -- takes its row index through
//     min(row, n - 1) before the address is computed, and the loads are unconditional on that clamped row; zeroing happens after the load, on the
//     value.  The largest row read is therefore b n + n - 1 for every workgroup, including the last sample of a full max_batch, behind which the
//     allocation ends.  Stores go to rows < n of the sample only.
__global__ __launch_bounds__(256) void clip_vis_attn_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out, int n, int W, int NT, int vpitch) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    bf16* Ks = reinterpret_cast<bf16*>(smem_raw);                        // [NT * 32][kKPitch]
    bf16* Vt = Ks + (size_t)NT * 32 * kKPitch;                           // [64][vpitch]
    const int hd = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const size_t ld = (size_t)3 * W;
    const bf16* base = qkv + (size_t)b * n * ld + hd * 64;               // row 0 of the sample, this head's q columns

    // stage K and V^T: item = (key j, 8-feature chunk c)
    for (int it = tid; it < NT * 32 * 8; it += 256) {
        const int j = it >> 3, c = it & 7;
        const int jr = j < n ? j : n - 1;                                // clamped BEFORE the address is formed
        const bf16* row = base + (size_t)jr * ld + c * 8;
        bf16x8 kv = *reinterpret_cast<const bf16x8*>(row + W);
        bf16x8 vv = *reinterpret_cast<const bf16x8*>(row + 2 * W);
        if (j >= n) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { kv[e] = (bf16)0.f; vv[e] = (bf16)0.f; }
        }
        *reinterpret_cast<bf16x8*>(Ks + (size_t)j * kKPitch + c * 8) = kv;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(size_t)(c * 8 + e) * vpitch + j] = vv[e];
    }
    __syncthreads();

    for (int qt = wave; qt < NT; qt += 4) {
        const int q = qt * 32 + r;
        const int qr = q < n ? q : n - 1;                                // clamped BEFORE the address is formed
        bf16x8 qf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(base + (size_t)qr * ld + s * 16 + 8 * h);

        f32x16 sc[kMaxKeyTiles];
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < kMaxKeyTiles; ++t) {
            if (t < NT) {
                f32x16 acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(Ks + (size_t)(t * 32 + r) * kKPitch + s * 16 + 8 * h);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[s], acc, 0, 0, 0);
                }
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                    const float v = key < n ? acc[i] * 0.125f : -INFINITY;
                    acc[i] = v;
                    m = fmaxf(m, v);
                }
                sc[t] = acc;
            }
        }
        m = fmaxf(m, __shfl_xor(m, 32, 64));                             // the other half of this query's keys (key 0 is always real: m is finite)
        float l = 0.f;
        f32x16 o0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o1 = o0;
#pragma unroll
        for (int t = 0; t < kMaxKeyTiles; ++t) {
            if (t < NT) {
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    bf16x8 pf;
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int i = 8 * s + j;
                        const int key = t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
                        const float e = key < n ? __expf(sc[t][i] - m) : 0.f;
                        l += e;
                        pf[j] = (bf16)e;
                    }
                    const int k0 = t * 32 + 16 * s + 4 * h;              // keys k0 .. k0 + 3 and k0 + 8 .. k0 + 11: the accumulator's own row order
                    const bf16x4 a0 = *reinterpret_cast<const bf16x4*>(Vt + (size_t)r * vpitch + k0);
                    const bf16x4 a1 = *reinterpret_cast<const bf16x4*>(Vt + (size_t)r * vpitch + k0 + 8);
                    const bf16x4 b0 = *reinterpret_cast<const bf16x4*>(Vt + (size_t)(32 + r) * vpitch + k0);
                    const bf16x4 b1 = *reinterpret_cast<const bf16x4*>(Vt + (size_t)(32 + r) * vpitch + k0 + 8);
                    const bf16x8 v0 = {a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
                    const bf16x8 v1 = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
                    o0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v0, pf, o0, 0, 0, 0);
                    o1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v1, pf, o1, 0, 0, 0);
                }
            }
        }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.0f / l;
        if (q < n) {
            bf16* orow = out + ((size_t)b * n + q) * W + hd * 64;
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d0 = 8 * g4 + 4 * h;                            // registers 4 g4 .. 4 g4 + 3 are features d0 .. d0 + 3 (+32 for o1)
                bf16x4 w0, w1;
#pragma unroll
                for (int e = 0; e < 4; ++e) { w0[e] = (bf16)(o0[4 * g4 + e] * inv); w1[e] = (bf16)(o1[4 * g4 + e] * inv); }
                *reinterpret_cast<bf16x4*>(orow + d0) = w0;
                *reinterpret_cast<bf16x4*>(orow + 32 + d0) = w1;
            }
        }
    }
}

size_t attn_lds_bytes(int NT) { return ((size_t)NT * 32 * kKPitch + (size_t)64 * v_pitch(NT * 32)) * sizeof(bf16); }

// one workgroup per (head, sample); the dynamic LDS follows the sample's own tile count
void launch_attention(const bf16* qkv, bf16* out, int batch, int n, int heads, hipStream_t s) {
    const int NT = (n + 31) / 32;
    static PerDeviceOnce attr_set;
    attr_set.run([&] {
        hipFuncSetAttribute(reinterpret_cast<const void*>(clip_vis_attn_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)attn_lds_bytes(kMaxKeyTiles));
    });
    hipLaunchKernelGGL(clip_vis_attn_kernel, dim3(heads, batch), dim3(256), attn_lds_bytes(NT), s, qkv, out, n, heads * 64, NT, v_pitch(NT * 32));
}

template <typename T>
void launch_im2col(const void* pix, bf16* rows, long total, int g, int p, int Kp, hipStream_t s) {
    hipLaunchKernelGGL(clip_vis_im2col_kernel<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, static_cast<const T*>(pix), rows, total, g, p, Kp);
}

}  // namespace

struct tld_clip_vis : ClipCore {              // the transformer, its workspace and the stage hook: tld_clip_core.h
    int g = 0, p = 0, n = 0, Kp = 0;          // n = g*g + 1 tokens; Kp = 3 p*p rounded up to a multiple of 64
    float *cls = nullptr, *pos = nullptr, *pre_g = nullptr, *pre_b = nullptr, *post_g = nullptr, *post_b = nullptr;
    bf16* conv_w = nullptr;                   // conv1.weight packed [W][Kp], zero beyond 3 p*p
    bf16* patches = nullptr;                  // workspace: max_batch * g*g rows of Kp
};

namespace {

// the tower's own GEMM operand beside the core's (name_operands): nothing before the weights exist
void name_conv_w(tld_clip_vis* c) { c->stages.ref("conv_w", c->conv_w, ST_BF16, c->W, c->Kp); }

}  // namespace

extern "C" {

int tld_clip_vis_create(const tld_clip_vis_config* cfg, tld_clip_vis** out) {
    if (!cfg || !out) return fail(TLD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (int rc = check_transformer(cfg->width, cfg->heads, cfg->layers)) return rc;
    if (cfg->patch_size < 1 || cfg->patch_size > 32) return fail(TLD_ERR_INVALID, "patch_size=%d: 1..32", cfg->patch_size);
    if (cfg->image_size < 1 || cfg->image_size % cfg->patch_size)
        return fail(TLD_ERR_INVALID, "image_size=%d: a positive multiple of patch_size=%d", cfg->image_size, cfg->patch_size);
    const int g = cfg->image_size / cfg->patch_size;
    if (g < 1 || g > kMaxGrid)
        return fail(TLD_ERR_INVALID, "image_size / patch_size = %d: the grid side must be 1..%d (at most %d tokens); the 336 px towers (577 tokens) are out of scope",
                    g, kMaxGrid, kMaxGrid * kMaxGrid + 1);
    if (cfg->embed_dim < 1 || cfg->max_batch < 1) return fail(TLD_ERR_INVALID, "embed_dim / max_batch must be positive");
    if (const std::string bad = clip_reach_check(cfg->max_batch, g * g + 1, cfg->width, g * g, (3 * cfg->patch_size * cfg->patch_size + 63) / 64 * 64); !bad.empty())
        return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    if (int rc = check_device(cfg->device_id, "image")) return rc;
    DeviceGuard guard(cfg->device_id);
    tld_clip_vis* c = new tld_clip_vis();
    c->W = cfg->width; c->L = cfg->layers; c->H = cfg->heads; c->E = cfg->embed_dim; c->max_batch = cfg->max_batch; c->device_id = cfg->device_id;
    c->g = g; c->p = cfg->patch_size; c->n = g * g + 1;
    c->Kp = (3 * c->p * c->p + 63) / 64 * 64;
    if (int rc = alloc_workspace(c, c->n, &c->patches, (size_t)cfg->max_batch * g * g * c->Kp)) { tld_clip_vis_destroy(c); return rc; }
    *out = c;
    return TLD_OK;
}

int tld_clip_vis_load_tensor(tld_clip_vis* c, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
    return load_tensor(c, CLIP_IMAGE, key, host_ptr, shape, ndim, dtype);
}

int tld_clip_vis_finalize_weights(tld_clip_vis* c) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    if (c->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    DeviceGuard guard(c->device_id);
    const int W = c->W, p = c->p, Kp = c->Kp;
    if (int rc = upload_entry(c, "visual.class_embedding", {W}, &c->cls)) return rc;
    if (int rc = upload_entry(c, "visual.positional_embedding", {c->n, W}, &c->pos)) return rc;
    if (int rc = upload_entry(c, "visual.ln_pre.weight", {W}, &c->pre_g)) return rc;
    if (int rc = upload_entry(c, "visual.ln_pre.bias", {W}, &c->pre_b)) return rc;
    if (int rc = upload_entry(c, "visual.ln_post.weight", {W}, &c->post_g)) return rc;
    if (int rc = upload_entry(c, "visual.ln_post.bias", {W}, &c->post_b)) return rc;
    if (int rc = upload_proj_t(c, "visual.proj")) return rc;
    const HostTensor* t = nullptr;
    if (int rc = need(c, "visual.conv1.weight", {W, 3, p, p}, &t)) return rc;
    {
        const int K0 = 3 * p * p;
        std::vector<float> cw((size_t)W * Kp, 0.f);
        for (int o = 0; o < W; ++o) for (int k = 0; k < K0; ++k) cw[(size_t)o * Kp + k] = t->data[(size_t)o * K0 + k];
        if (int rc = upload_bf16(c, cw, &c->conv_w)) return rc;
    }
    if (int rc = upload_blocks(c, CLIP_IMAGE)) return rc;
    if (int rc = finish_weights(c)) return rc;
    name_conv_w(c);
    return TLD_OK;
}

int tld_clip_vis_encode_image(tld_clip_vis* c, const void* pixels, float* out, int32_t batch, int32_t io_dtype, void* hip_stream) {
    if (!c || !pixels || !out) return fail(TLD_ERR_INVALID, "null argument");
    if (int rc = check_encode(c, batch)) return rc;
    if (io_dtype != TLD_DTYPE_F32 && io_dtype != TLD_DTYPE_BF16 && io_dtype != TLD_DTYPE_F16) return fail(TLD_ERR_INVALID, "io_dtype=%d: fp32, bf16 or fp16", io_dtype);
    DeviceGuard guard(c->device_id);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int W = c->W, n = c->n, g = c->g, Kp = c->Kp, T = batch * n, P = batch * g * g;
    if (c->debug) { if (int rc = begin_debug_call(c, n, "tld_clip_vis_set_debug", s, c->patches, (size_t)c->max_batch * g * g * Kp)) return rc; }
    {
        const long total = (long)P * Kp;
        if (io_dtype == TLD_DTYPE_F32) launch_im2col<float>(pixels, c->patches, total, g, c->p, Kp, s);
        else if (io_dtype == TLD_DTYPE_BF16) launch_im2col<bf16>(pixels, c->patches, total, g, c->p, Kp, s);
        else launch_im2col<_Float16>(pixels, c->patches, total, g, c->p, Kp, s);
    }
    CLIP_KEEP("patches", c->patches, ST_BF16, P, Kp);
    GEMM_TRY("tld_clip_vis_encode_image, patch embedding conv1", gemm(c->patches, Kp, c->conv_w, P, W, Kp, EPI_F32, nullptr, nullptr, c->tmp, s));
    CLIP_KEEP("emb", c->tmp, ST_F32, P, W);
    hipLaunchKernelGGL(clip_vis_embed_ln_kernel, dim3((T + 3) / 4), dim3(256), 0, s, c->tmp, c->cls, c->pos, c->pre_g, c->pre_b, c->x, T, W, n);
    // the class token's row of each sample is the pooled one (no EOT index), through ln_post
    auto attention = [&] { launch_attention(c->qkv, c->att, batch, n, c->H, s); };
    if (int rc = run_blocks(c, batch, n, attention, nullptr, c->post_g, c->post_b, "tld_clip_vis_encode_image", out, s)) return rc;
    return check_launch("encode_image");
}

int tld_clip_vis_set_debug(tld_clip_vis* c, int32_t enable) {
    if (!c) return fail(TLD_ERR_INVALID, "null handle");
    DeviceGuard guard(c->device_id);
    if (!enable) { drop_snapshots(c); name_conv_w(c); return TLD_OK; }
    if (c->debug) return TLD_OK;
    const size_t P = (size_t)c->max_batch * c->g * c->g;
    int rc = c->stages.reserve("patches", P * c->Kp * 2);
    if (!rc) rc = c->stages.reserve("emb", P * c->W * 4);
    if (!rc) rc = reserve_stages(c, c->n);
    if (rc) {
        drop_snapshots(c);
        name_conv_w(c);
        return fail(TLD_ERR_HIP, "tld_clip_vis_set_debug: no memory for the stage snapshots of %d images x %d layers; debug stays off", c->max_batch, c->L);
    }
    c->debug = true;
    return TLD_OK;
}

int tld_clip_vis_read_stage(tld_clip_vis* c, const char* name, float* host_out, int64_t numel, int64_t* shape4) { return read_stage(c, name, host_out, numel, shape4); }

int tld_debug_clip_vis_attention(const void* qkv_bf16, void* out_bf16, int32_t batch, int32_t n, int32_t heads, void* hip_stream) {
    if (!qkv_bf16 || !out_bf16) return fail(TLD_ERR_INVALID, "null argument");
    if (batch < 1 || batch > 65535) return fail(TLD_ERR_INVALID, "batch=%d: 1..65535", batch);
    if (n < 2 || n > kMaxGrid * kMaxGrid + 1) return fail(TLD_ERR_INVALID, "n=%d tokens: 2..%d", n, kMaxGrid * kMaxGrid + 1);
    if (heads < 1 || heads > 16) return fail(TLD_ERR_INVALID, "heads=%d: 1..16 (width = 64 heads <= 1024)", heads);
    PtrDeviceGuard guard(qkv_bf16);
    launch_attention(static_cast<const bf16*>(qkv_bf16), static_cast<bf16*>(out_bf16), batch, n, heads, reinterpret_cast<hipStream_t>(hip_stream));
    return check_launch("tld_debug_clip_vis_attention");
}

int64_t tld_clip_vis_weight_bytes(const tld_clip_vis* c) { return weight_bytes(c); }

int tld_clip_vis_destroy(tld_clip_vis* c) {
    if (!c) return TLD_OK;
    release(c);
    delete c;
    return TLD_OK;
}

}  // extern "C"

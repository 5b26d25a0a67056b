// tld_batch.hip -- the training batch of one step, built on the device from a resident latent dataset (tld_train_prepare_batch; DESIGN.md
// section 7.11): what Trainer.make_batch does on the host (tld/train.py:121-138) as ONE kernel -- gather the rows idx[b], dequantise, draw the
// noise, the noise level and the label mask from Philox4x32-10 (tld_batch_math.h), mix in double.
//
// Geometry: sample b owns `chunks` consecutive workgroups of 256 lanes; they walk the Philox counters that cover the sample's flat elements
// [b E, (b + 1) E) and its label row.  Every draw is addressed by (seed, replica, step, position) through the counter, so neither `chunks` nor the
// workgroup size shows in the result.  Each workgroup first derives its sample's three scalars on three different waves -- lane 0: ln Gamma(a),
// lane 64: ln Gamma(b), lane 128: the checked row index and the label mask -- and shares them through LDS; the Beta draw is
// 1 / (1 + exp(ln Gamma(b) - ln Gamma(a))), evaluated by every lane alike.  All stores are ordinary vector stores; the one atomic is a global
// (vector-memory) atomic add.
#include "tld_common.h"
#include "tld_host.h"        // fail, DeviceGuard, HIP_TRY
#include "tld_batch_math.h"
#include "tld_normal_device.h"     // log_uniform24_open
#include "../../include/tld_hip.h"

#include <algorithm>
#include <cmath>

namespace tld {

namespace {

constexpr int kBatchLanes = 256;
constexpr int kBatchMaxChunks = 64;

struct BatchArgs {
    const void* latents; const void* labels; const float* table; const int64_t* idx;
    float *x_noisy, *noise_level, *label, *target, *noise;
    double* noise_level64; uint8_t* mask; int32_t* bad;
    const double* level_in;                               // given noise levels [batch] (tld_train_prepare_batch_at); null: the Beta draw
    int64_t rows; uint64_t seed, step;
    double beta_a, beta_b;
    float vae_scale, label_dropout;
    uint32_t replica;
    int32_t lat_dtype, lab_dtype, E, text, chunks, vec;
};

// ln of one Gamma(shape, 1) draw of sample b: Marsaglia & Tsang (ACM TOMS 26(3), 2000) for shape >= 1; below 1 it is Gamma(shape + 1) U^(1 / shape),
// added in the logarithm so that a tiny shape cannot underflow.  Attempt j reads counter 64 b + base + j: a normal by Box-Muller from 53 + 32 bits, the
// acceptance uniform from the last 32.  At most BATCH_GAMMA_TRIES attempts (each accepts with probability > 0.95 for every shape >= 1, so all fail with
// probability < 0.05^16 = 1.6e-21); then the draw is d = shape - 1/3, the value at x = 0.
__device__ double log_gamma_draw(double shape, uint32_t base, const BatchArgs& A, uint32_t b) {
    const bool boost = shape < 1.0;
    const double a1 = boost ? shape + 1.0 : shape;
    const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
    const uint32_t c0 = BATCH_LEVEL_SLOTS * b + base;
    double g = d;
    for (int j = 0; j < BATCH_GAMMA_TRIES; ++j) {
        const Philox4 p = batch_philox(A.seed, A.step, A.replica, BATCH_STREAM_LEVEL, c0 + (uint32_t)j);
        const double x = sqrt(-2.0 * log(uniform53_open(p.v[0], p.v[1]))) * cospi(2.0 * uniform32_open(p.v[2]));
        double v = 1.0 + c * x;
        if (v <= 0.0) continue;
        v = v * v * v;
        if (log(uniform32_open(p.v[3])) < 0.5 * x * x + d - d * v + d * log(v)) { g = d * v; break; }
    }
    double lg = log(g);
    if (boost) {
        const Philox4 p = batch_philox(A.seed, A.step, A.replica, BATCH_STREAM_LEVEL, c0 + (uint32_t)BATCH_GAMMA_TRIES);
        lg += log(uniform53_open(p.v[0], p.v[1])) / shape;
    }
    return lg;
}

__device__ __forceinline__ float half_bits_to_float(uint16_t h) {
    return (float)__builtin_bit_cast(_Float16, h);
}

// target of one source element: the table for codes, a correctly rounded division for floats
__device__ __forceinline__ float dequant_u8(const float* tab, uint8_t c) { return tab[c]; }
__device__ __forceinline__ float scaled(float v, float scale) { return __fdiv_rn(v, scale); }

__device__ __forceinline__ float mix(double nl, double sl, float noise, float target) {
    return (float)__dadd_rn(__dmul_rn(nl, (double)noise), __dmul_rn(sl, (double)target));
}

__global__ __launch_bounds__(kBatchLanes) void prepare_batch_kernel(BatchArgs A) {
#pragma clang fp contract(off)
    __shared__ float tab[256];
    __shared__ double sh_lg[2];
    __shared__ int64_t sh_row;
    __shared__ int sh_drop;
    const int tid = threadIdx.x;
    const uint32_t b = blockIdx.x / (uint32_t)A.chunks, chunk = blockIdx.x % (uint32_t)A.chunks;

    if (A.lat_dtype == TLD_DTYPE_U8) tab[tid] = A.table[tid];
    if (!A.level_in) {
        if (tid == 0) sh_lg[0] = log_gamma_draw(A.beta_a, 0, A, b);
        if (tid == 64) sh_lg[1] = log_gamma_draw(A.beta_b, BATCH_LEVEL_SLOTS / 2, A, b);
    }
    if (tid == 128) {
        int64_t r = A.idx[b];
        if (r < 0 || r >= A.rows) {                       // never dereferenced: the position takes row 0, and the call says so
            r = 0;
            if (chunk == 0) atomicAdd(A.bad, 1);
        }
        sh_row = r;
        const Philox4 p = batch_philox(A.seed, A.step, A.replica, BATCH_STREAM_MASK, b >> 2);
        const uint32_t w = (b & 2) ? ((b & 1) ? p.v[3] : p.v[2]) : ((b & 1) ? p.v[1] : p.v[0]);      // (selects: an indexed p.v[b & 3] costs an LDS array)
        sh_drop = uniform24(w) < A.label_dropout ? 1 : 0;
    }
    __syncthreads();
    double nl;
    if (A.level_in) nl = A.level_in[b];                   // used as given: a NaN propagates
    else nl = 1.0 / (1.0 + exp(sh_lg[1] - sh_lg[0]));
    const double sl = __dsub_rn(1.0, nl);
    const int64_t row = sh_row;
    const int drop = sh_drop;
    if (chunk == 0 && tid == 0) {
        A.noise_level[b] = (float)nl;
        if (A.noise_level64) A.noise_level64[b] = nl;
        if (A.mask) A.mask[b] = (uint8_t)drop;
    }

    // ---- the label row: scalar loads (a row of fp16 values need not be aligned to anything wider) --------------------------------------------
    {
        const int64_t src = row * A.text, dst = (int64_t)b * A.text;
        for (int j = (int)chunk * kBatchLanes + tid; j < A.text; j += A.chunks * kBatchLanes) {
            float v = 0.f;
            if (!drop) v = A.lab_dtype == TLD_DTYPE_F32 ? static_cast<const float*>(A.labels)[src + j]
                                                         : half_bits_to_float(static_cast<const uint16_t*>(A.labels)[src + j]);
            A.label[dst + j] = v;
        }
    }

    // ---- the latent row: one Philox counter = four flat elements --------------------------------------------------------------------------------
    const int64_t e_lo = (int64_t)b * A.E, e_hi = e_lo + A.E, src0 = row * A.E - e_lo;        // source element of flat element e: src0 + e
    const int64_t q_hi = (e_hi + 3) >> 2;
    for (int64_t q = (e_lo >> 2) + (int64_t)chunk * kBatchLanes + tid; q < q_hi; q += (int64_t)A.chunks * kBatchLanes) {
        const Philox4 p = batch_philox(A.seed, A.step, A.replica, BATCH_STREAM_NOISE, (uint32_t)q);
        float n[4];
        for (int h = 0; h < 2; ++h) {
            const float rad = __fsqrt_rn(-2.f * log_uniform24_open(p.v[2 * h]));
            float sn, cs;
            sincospif(2.f * uniform24_open(p.v[2 * h + 1]), &sn, &cs);
            n[2 * h] = rad * cs;
            n[2 * h + 1] = rad * sn;
        }
        const int64_t e = q << 2;
        if (A.vec) {                                      // E % 4 == 0 and every pointer aligned for its 4-element access: the quad lies in the row
            float t[4];
            if (A.lat_dtype == TLD_DTYPE_U8) {
                const uchar4 c = *reinterpret_cast<const uchar4*>(static_cast<const uint8_t*>(A.latents) + src0 + e);
                t[0] = dequant_u8(tab, c.x); t[1] = dequant_u8(tab, c.y); t[2] = dequant_u8(tab, c.z); t[3] = dequant_u8(tab, c.w);
            } else if (A.lat_dtype == TLD_DTYPE_F16) {
                const ushort4 c = *reinterpret_cast<const ushort4*>(static_cast<const uint16_t*>(A.latents) + src0 + e);
                t[0] = scaled(half_bits_to_float(c.x), A.vae_scale); t[1] = scaled(half_bits_to_float(c.y), A.vae_scale);
                t[2] = scaled(half_bits_to_float(c.z), A.vae_scale); t[3] = scaled(half_bits_to_float(c.w), A.vae_scale);
            } else {
                const float4 c = *reinterpret_cast<const float4*>(static_cast<const float*>(A.latents) + src0 + e);
                t[0] = scaled(c.x, A.vae_scale); t[1] = scaled(c.y, A.vae_scale); t[2] = scaled(c.z, A.vae_scale); t[3] = scaled(c.w, A.vae_scale);
            }
            *reinterpret_cast<float4*>(A.target + e) = make_float4(t[0], t[1], t[2], t[3]);
            *reinterpret_cast<float4*>(A.x_noisy + e) = make_float4(mix(nl, sl, n[0], t[0]), mix(nl, sl, n[1], t[1]), mix(nl, sl, n[2], t[2]), mix(nl, sl, n[3], t[3]));
            if (A.noise) *reinterpret_cast<float4*>(A.noise + e) = make_float4(n[0], n[1], n[2], n[3]);
        } else {
            for (int k = 0; k < 4; ++k) {
                const int64_t ek = e + k;
                if (ek < e_lo || ek >= e_hi) continue;    // a counter that straddles two samples: each sample's workgroups store their own part
                float t;
                if (A.lat_dtype == TLD_DTYPE_U8) t = dequant_u8(tab, static_cast<const uint8_t*>(A.latents)[src0 + ek]);
                else if (A.lat_dtype == TLD_DTYPE_F16) t = scaled(half_bits_to_float(static_cast<const uint16_t*>(A.latents)[src0 + ek]), A.vae_scale);
                else t = scaled(static_cast<const float*>(A.latents)[src0 + ek], A.vae_scale);
                A.target[ek] = t;
                A.x_noisy[ek] = mix(nl, sl, n[k], t);
                if (A.noise) A.noise[ek] = n[k];
            }
        }
    }
}

}  // namespace

}  // namespace tld

using namespace tld;

extern "C" {

int tld_train_prepare_batch(tld_train* e, const tld_batch_source* src, const int64_t* idx, int32_t batch, uint64_t seed, uint64_t step, uint32_t replica,
                            double beta_a, double beta_b, float label_dropout, float* x_noisy, float* noise_level, float* label, float* target, float* noise,
                            double* noise_level64, uint8_t* mask, int32_t* bad_index_count, void* hip_stream) {
    return tld_train_prepare_batch_at(e, src, idx, batch, seed, step, replica, beta_a, beta_b, label_dropout, x_noisy, noise_level, label, target, noise, noise_level64,
                                      mask, bad_index_count, hip_stream, nullptr);
}

int tld_train_prepare_batch_at(tld_train* e, const tld_batch_source* src, const int64_t* idx, int32_t batch, uint64_t seed, uint64_t step, uint32_t replica,
                               double beta_a, double beta_b, float label_dropout, float* x_noisy, float* noise_level, float* label, float* target, float* noise,
                               double* noise_level64, uint8_t* mask, int32_t* bad_index_count, void* hip_stream, const double* noise_level_in) {
    (void)e;                                              // no engine state is read: the handle is accepted for symmetry with the other tld_train_* entries
    if (!src || !src->latents || !src->labels || !idx) return fail(TLD_ERR_INVALID, "prepare batch: null source or index pointer");
    if (!x_noisy || !noise_level || !label || !target || !bad_index_count) return fail(TLD_ERR_INVALID, "prepare batch: null output pointer");
    if (batch <= 0 || src->rows <= 0 || src->latent_elems <= 0 || src->text_emb <= 0)
        return fail(TLD_ERR_INVALID, "prepare batch: batch %d, rows %lld, latent_elems %d, text_emb %d", batch, (long long)src->rows, src->latent_elems, src->text_emb);
    if (batch > (1 << 26) || (int64_t)batch * src->latent_elems > ((int64_t)1 << 34))
        return fail(TLD_ERR_INVALID, "prepare batch: batch %d x %d elements exceeds the 32-bit Philox counter (batch <= 2^26, batch * elements <= 2^34)", batch,
                    src->latent_elems);
    const int lt = src->latent_dtype, bt = src->label_dtype;
    if (lt != TLD_DTYPE_U8 && lt != TLD_DTYPE_F16 && lt != TLD_DTYPE_F32) return fail(TLD_ERR_INVALID, "prepare batch: latent dtype %d (uint8, fp16 or fp32)", lt);
    if (bt != TLD_DTYPE_F16 && bt != TLD_DTYPE_F32) return fail(TLD_ERR_INVALID, "prepare batch: label dtype %d (fp16 or fp32)", bt);
    if (lt == TLD_DTYPE_U8 && !src->dequant_table) return fail(TLD_ERR_INVALID, "prepare batch: uint8 latents need a dequantisation table");
    if (lt != TLD_DTYPE_U8 && !(std::isfinite(src->vae_scale) && src->vae_scale != 0.f))
        return fail(TLD_ERR_INVALID, "prepare batch: vae_scale %g", (double)src->vae_scale);
    if (!(beta_a > 0.0) || !(beta_b > 0.0) || std::isinf(beta_a) || std::isinf(beta_b))
        return fail(TLD_ERR_INVALID, "prepare batch: Beta(%g, %g) needs finite shapes > 0", beta_a, beta_b);
    if (!(label_dropout >= 0.f && label_dropout <= 1.f)) return fail(TLD_ERR_INVALID, "prepare batch: label_dropout %g outside [0, 1]", (double)label_dropout);
    if ((uintptr_t)noise_level_in & 7) return fail(TLD_ERR_INVALID, "prepare batch: noise_level_in must be 8-byte aligned");

    BatchArgs A{};
    A.latents = src->latents; A.labels = src->labels; A.table = src->dequant_table; A.idx = idx;
    A.x_noisy = x_noisy; A.noise_level = noise_level; A.label = label; A.target = target; A.noise = noise;
    A.noise_level64 = noise_level64; A.mask = mask; A.bad = bad_index_count; A.level_in = noise_level_in;
    A.rows = src->rows; A.seed = seed; A.step = step; A.beta_a = beta_a; A.beta_b = beta_b;
    A.vae_scale = src->vae_scale; A.label_dropout = label_dropout; A.replica = replica;
    A.lat_dtype = lt; A.lab_dtype = bt; A.E = src->latent_elems; A.text = src->text_emb;
    const int quads = (A.E + 3) / 4 + 1, work = std::max(quads, A.text);
    A.chunks = std::min(kBatchMaxChunks, (work + kBatchLanes - 1) / kBatchLanes);
    const uintptr_t src_align = lt == TLD_DTYPE_U8 ? 3 : lt == TLD_DTYPE_F16 ? 7 : 15;
    A.vec = A.E % 4 == 0 && !(((uintptr_t)x_noisy | (uintptr_t)target | (uintptr_t)noise) & 15) && !((uintptr_t)src->latents & src_align);

    DeviceGuard dg(std::max(0, ptr_device(x_noisy)));
    hipLaunchKernelGGL(prepare_batch_kernel, dim3((uint32_t)batch * (uint32_t)A.chunks), dim3(kBatchLanes), 0, reinterpret_cast<hipStream_t>(hip_stream), A);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

}  // extern "C"

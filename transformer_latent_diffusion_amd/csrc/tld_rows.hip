// tld_rows.hip -- the HBM-bound row kernels of the denoiser (wavefront reductions, coalesced rows).
//
//   embed_kernel        patchify conv + LN(pd) + Linear(pd->d) + LN(d) + pos-embed   tld/denoiser.py:34-45,75-77
//   layernorm_bf16      LayerNorm rows -> bf16 GEMM operand                           tld/transformer_blocks.py:131,136
//   cross_row_kernel    SA residual add + whole cross-attention sub-block + LN3       tld/transformer_blocks.py:136-138, 62-72
//   tail_kernel         out_proj Linear(d->pd) + unpatchify                           tld/denoiser.py:47-52,72,82
//   sampler_step_kernel CFG combine + DPM-Solver++(2M)/DDIM update + latent shifts    tld/diffusion.py:66-89,122-125
//                       (+ the inpainting blend), per-sample scalars from a device table: the one step of all three sampler entries
//   start_mix_kernel    x_start = s0 eps + (1 - s0) z0, the forward process of tld/train.py:130, s0 per sample from a device table
//   dwconv_gelu_kernel  depthwise 3x3 + bias + exact GELU, channels-last              tld/transformer_blocks.py:96-103
//
// Row layout: a wave owns one token row of d features; lane l holds features {2l, 2l+1} + 128*j
// (float2 per access, 512 B per wave-instruction).  d = 128 NJ, or 128 NJ - 64 (template flag HALF: embed_dim is any
// multiple of the head width 64, transformer_blocks.py:126-128): the last group then holds 64 features in lanes 0-31
// and lanes 32-63 carry zeros through every sum and skip their loads / stores (`live`).
#include "tld_common.h"
#include "tld_sampler_noise.h"    // the counter of the stochastic sampler's noise
#include "tld_normal_device.h"    // philox_normals4
#include <cstdlib>
#include <type_traits>

namespace tld {

namespace {


// ------------------------------------------------------------------------------------------------
// Workgroup = 32 token rows (8 per wave); the Linear(pd -> d) weight table [pd][d] fp32 (49 KB at d = 768)
// is staged in LDS once per workgroup -- read per row from L1/L2 it made the kernel L1-bandwidth bound.
template <int NJ, bool HALF>
__global__ __launch_bounds__(256) void embed_kernel(EmbedParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int d = NJ * 128 - (HALF ? 64 : 0);
    float* wt = reinterpret_cast<float*>(smem);                  // [pd][d]
    float* cwt = wt + p.pd * d;                                  // [C p p][pd]  conv weight, transposed (lane = output)
    for (int i = threadIdx.x; i < p.pd * d / 4; i += 256)
        reinterpret_cast<float4*>(wt)[i] = reinterpret_cast<const float4*>(p.lin_wt)[i];
    for (int i = threadIdx.x; i < p.pd * p.C * p.p * p.p; i += 256) {
        const int o = i / (p.C * p.p * p.p), k = i - o * (p.C * p.p * p.p);
        cwt[k * p.pd + o] = p.conv_w[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live_last = !HALF || lane < 32;                   // does this lane hold features of the last 128-group?
    auto live = [&](int j) { return j + 1 < NJ || live_last; };
    const int pp = p.p * p.p, cpp = p.C * pp;
    const int total = p.batch * p.ntok;
    // per-lane constants
    const float cb = lane < p.pd ? p.conv_b[lane] : 0.f;
    const float* cw = cwt + (lane < p.pd ? lane : 0);            // + i * pd
    const float g1 = lane < p.pd ? p.ln1_w[lane] : 0.f, b1 = lane < p.pd ? p.ln1_b[lane] : 0.f;
    const int ic = lane / pp, iuv = lane - ic * pp, iu = iuv / p.p, iv = iuv - iu * p.p;   // lane = (c,u,v) for loads
    // 8 rows per wave, two workgroups per CU at the bench size: with 16 rows per wave and one workgroup per CU the
    // kernel was bound by the latency of each row's input load (90 us for 16 K rows); the next row's load is issued early
    constexpr int ROWS_PER_WAVE = 8;
    auto load_in = [&](int row) {
        float xv = 0.f;
        if (row < total && lane < cpp) {
            const int b = row / p.ntok, t = row - b * p.ntok;
            const int ti = t / p.grid, tj = t - ti * p.grid;
            xv = p.x[(((size_t)(p.src_row ? p.src_row[b] : b % p.src_batch) * p.C + ic) * p.S + (ti * p.p + iu)) * p.S + (tj * p.p + iv)];
        }
        return xv;
    };
    const int row_first = (blockIdx.x * 4 + wid) * ROWS_PER_WAVE;
    float xnext = load_in(row_first);
    for (int rr = 0; rr < ROWS_PER_WAVE; ++rr) {
        const int row = row_first + rr;
        if (row >= total) return;
        const int t = row % p.ntok;
        const float xin = xnext;
        if (rr + 1 < ROWS_PER_WAVE) xnext = load_in(row + 1);
        // (both small loops are unrolled by hand -- `#pragma unroll` refuses loops around v_readlane -- so that the
        // LDS reads of four taps are in flight together; they were one exposed LDS latency per tap)
        float pv = cb;
        {
            int i = 0;
            for (; i + 4 <= cpp; i += 4) {
                const float c0 = cw[(i + 0) * p.pd], c1 = cw[(i + 1) * p.pd], c2 = cw[(i + 2) * p.pd], c3 = cw[(i + 3) * p.pd];
                pv = fmaf(c0, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xin), i + 0)), pv);
                pv = fmaf(c1, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xin), i + 1)), pv);
                pv = fmaf(c2, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xin), i + 2)), pv);
                pv = fmaf(c3, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xin), i + 3)), pv);
            }
            for (; i < cpp; ++i)
                pv = fmaf(cw[i * p.pd], __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xin), i)), pv);
        }
        if (lane >= p.pd) pv = 0.f;
        const float inv_pd = 1.0f / (float)p.pd;
        const float mean1 = wave_sum(pv) * inv_pd;
        const float dv = lane < p.pd ? pv - mean1 : 0.f;
        const float rstd1 = 1.0f / sqrtf(wave_sum(dv * dv) * inv_pd + kLnEps);
        const float pn = dv * rstd1 * g1 + b1;                   // 0 for lanes >= pd

        float2 e[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) e[j] = live(j) ? *reinterpret_cast<const float2*>(p.lin_b + j * 128 + 2 * lane) : make_float2(0.f, 0.f);
        auto lin_tap = [&](int o, const float2 (&w)[NJ]) {
            const float a = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn), o));
#pragma unroll
            for (int j = 0; j < NJ; ++j) { e[j].x = fmaf(a, w[j].x, e[j].x); e[j].y = fmaf(a, w[j].y, e[j].y); }
        };
        auto lin_load = [&](int o, float2 (&w)[NJ]) {
            const float* wrow = wt + o * d + 2 * lane;
#pragma unroll
            for (int j = 0; j < NJ; ++j) w[j] = live(j) ? *reinterpret_cast<const float2*>(wrow + j * 128) : make_float2(0.f, 0.f);
        };
        {
            int o = 0;
            for (; o + 2 <= p.pd; o += 2) {
                float2 w0[NJ], w1[NJ];
                lin_load(o, w0); lin_load(o + 1, w1);
                lin_tap(o, w0); lin_tap(o + 1, w1);
            }
            if (o < p.pd) { float2 w0[NJ]; lin_load(o, w0); lin_tap(o, w0); }
        }
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) s += e[j].x + e[j].y;
        const float mean2 = wave_sum(s) / (float)d;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (live(j)) { e[j].x -= mean2; e[j].y -= mean2; }
            q += e[j].x * e[j].x + e[j].y * e[j].y;
        }
        const float rstd2 = 1.0f / sqrtf(wave_sum(q) / (float)d + kLnEps);
        float ssum = 0.f, ssq = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (!live(j)) continue;
            const int n = j * 128 + 2 * lane;
            const float2 g = *reinterpret_cast<const float2*>(p.ln2_w + n);
            const float2 bb = *reinterpret_cast<const float2*>(p.ln2_b + n);
            const float2 pe = *reinterpret_cast<const float2*>(p.pos + (size_t)t * d + n);
            float2 o;
            o.x = e[j].x * rstd2 * g.x + bb.x + pe.x;
            o.y = e[j].y * rstd2 * g.y + bb.y + pe.y;
            rs_store2(p.tok + (size_t)row * d + n, o);
            const float r0 = rs_round(o.x), r1 = rs_round(o.y);
            ssum += r0 + r1;
            ssq = fmaf(r0, r0, fmaf(r1, r1, ssq));
        }
        if (p.stats_out) {       // LayerNorm-1 statistics of block 0, consumed by its QKV GEMM epilogue (slots come in pairs)
            ssum = wave_sum(ssum); ssq = wave_sum(ssq);
            if (lane == 0) *reinterpret_cast<float4*>(p.stats_out + (size_t)row * kLnSlots) = make_float4(ssum, ssq, 0.f, 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------
template <int NJ, bool HALF>
__global__ __launch_bounds__(256) void layernorm_bf16_kernel(const resid_t* __restrict__ x,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ b,
                                                             bf16* __restrict__ out, int M, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bool live_last = !HALF || lane < 32;
    auto live = [&](int j) { return j + 1 < NJ || live_last; };
    float2 v[NJ];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        v[j] = live(j) ? rs_load2(x + (size_t)row * d + j * 128 + 2 * lane) : make_float2(0.f, 0.f);
        s += v[j].x + v[j].y;
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (live(j)) { v[j].x -= mean; v[j].y -= mean; }
        q += v[j].x * v[j].x + v[j].y * v[j].y;
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + kLnEps);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        if (!live(j)) continue;
        const int n = j * 128 + 2 * lane;
        const float2 gg = *reinterpret_cast<const float2*>(g + n);
        const float2 bb = *reinterpret_cast<const float2*>(b + n);
        bf16x2 o;
        o[0] = (bf16)(v[j].x * rstd * gg.x + bb.x);
        o[1] = (bf16)(v[j].y * rstd * gg.y + bb.y);
        *reinterpret_cast<bf16x2*>(out + (size_t)row * d + n) = o;
    }
}

// LayerNorm arithmetic of the 4-features-per-lane kernels, shared by the bf16 writer and the MX-fp8 writer: the two must produce the
// SAME bf16 values bit for bit (tests/test_gpu_fp8.py: quantising producers == separate passes).  Under HIP's -ffp-contract=fast the
// backend decides per context which multiply-adds fuse, so identical source in two kernels is not identical arithmetic (seen: one token
// row in ~5000 differing between the two at a LayerNorm-1); contraction is pinned here and the fused operations are spelled out.
template <int NQ>
__device__ __forceinline__ void ln_q4_stats(float4 (&v)[NQ], int d, float& rstd) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        v[j].x -= mean; v[j].y -= mean; v[j].z -= mean; v[j].w -= mean;
        q += __builtin_fmaf(v[j].x, v[j].x, v[j].y * v[j].y) + __builtin_fmaf(v[j].z, v[j].z, v[j].w * v[j].w);
    }
    rstd = 1.0f / sqrtf(wave_sum(q) / (float)d + kLnEps);
}
__device__ __forceinline__ float ln_q4_affine(float v, float rstd, float g, float b) {
#pragma clang fp contract(off)
    return __builtin_fmaf(v * rstd, g, b);
}

// d % 256 == 0 form: lane l holds features {4l .. 4l+3} + 256 j, i.e. 8-byte loads of the bf16 residual and 8-byte
// stores (the 2-feature layout above moves 4 bytes per lane and instruction)
template <int NQ>
__global__ __launch_bounds__(256) void layernorm_bf16_q4_kernel(const resid_t* __restrict__ x,
                                                                const float* __restrict__ g,
                                                                const float* __restrict__ b,
                                                                bf16* __restrict__ out, int M, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float4 v[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) v[j] = rs_load4(x + (size_t)row * d + j * 256 + 4 * lane);
    float rstd;
    ln_q4_stats<NQ>(v, d, rstd);
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int n = j * 256 + 4 * lane;
        const float4 gg = *reinterpret_cast<const float4*>(g + n);
        const float4 bb = *reinterpret_cast<const float4*>(b + n);
        bf16x4 o;
        o[0] = (bf16)ln_q4_affine(v[j].x, rstd, gg.x, bb.x);
        o[1] = (bf16)ln_q4_affine(v[j].y, rstd, gg.y, bb.y);
        o[2] = (bf16)ln_q4_affine(v[j].z, rstd, gg.z, bb.z);
        o[3] = (bf16)ln_q4_affine(v[j].w, rstd, gg.w, bb.w);
        *reinterpret_cast<bf16x4*>(out + (size_t)row * d + n) = o;
    }
}

// fp8 GEMM mode: the same LayerNorm rows written straight in the MX-fp8 operand format (no bf16 copy, no separate
// quantisation pass).  A 32-feature block is 8 adjacent lanes of one 256-feature chunk.
template <int NQ>
__global__ __launch_bounds__(256) void layernorm_mx8_kernel(const resid_t* __restrict__ x, const float* __restrict__ g,
                                                            const float* __restrict__ b, uint8_t* __restrict__ out8,
                                                            uint8_t* __restrict__ scale8, int M, int d) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float4 v[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) v[j] = rs_load4(x + (size_t)row * d + j * 256 + 4 * lane);
    float rstd;
    ln_q4_stats<NQ>(v, d, rstd);
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int n = j * 256 + 4 * lane;
        const float4 gg = *reinterpret_cast<const float4*>(g + n);
        const float4 bb = *reinterpret_cast<const float4*>(b + n);
        // (rounded through bf16 first: the operand the bf16 path would have produced is what gets quantised)
        const float y0 = (float)(bf16)ln_q4_affine(v[j].x, rstd, gg.x, bb.x), y1 = (float)(bf16)ln_q4_affine(v[j].y, rstd, gg.y, bb.y);
        const float y2 = (float)(bf16)ln_q4_affine(v[j].z, rstd, gg.z, bb.z), y3 = (float)(bf16)ln_q4_affine(v[j].w, rstd, gg.w, bb.w);
        int e8;
        const unsigned w = mx8_pack4(y0, y1, y2, y3, &e8);
        *reinterpret_cast<unsigned*>(out8 + (size_t)row * d + n) = w;
        if ((lane & 7) == 0) scale8[mx8_scale_index(n, (size_t)row, (size_t)M)] = (uint8_t)e8;
    }
}

// ------------------------------------------------------------------------------------------------
// Cross-attention has only two keys per sample (the noise token and the label token), so
//   softmax([q.k_n, q.k_l] / 8) = [1 - s, s],  s = sigmoid((q.k_l - q.k_n) / 8),
// and q.k_t / 8 = LN2(x) . (Wq_h^T k_t[h] / 8): the query projection folds into one d-vector per
// (token row, head), prepared once on the conditioning path (wq table, LN2 gamma folded in, LN2 beta
// contribution in bwq).  The sub-block therefore needs no GEMM: per row it is 12 dot products of
// the centred row against LDS-resident vectors, a sigmoid per head, and a blend of the two value rows.
template <int NJ, bool HALF>
__global__ __launch_bounds__(256, 3) void cross_row_kernel(CrossRowParams p, int chunks_per_sample) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int d = NJ * 128 - (HALF ? 64 : 0), H = d / 64;
    constexpr float inv_d = 1.0f / (float)d;
    float* wd = reinterpret_cast<float*>(smem);          // [H][d]  wq_label - wq_noise (gamma folded)
    float* vn = wd + H * d;                              // [d]     value row of the noise token
    float* vdiff = vn + d;                               // [d]     v_label - v_noise
    float* bw = vdiff + d;                               // [H]     beta contribution to the logit diff

    // A workgroup owns one contiguous chunk of ROW PAIRS of one sample (balanced split, so the grid can be sized
    // to exactly one resident round: 3 workgroups per CU); its four waves take the pairs round-robin.
    const int b = blockIdx.x / chunks_per_sample;
    const int ck = blockIdx.x - b * chunks_per_sample;
    const int pairs = p.ntok >> 1;
    const int pp0 = (int)((long)ck * pairs / chunks_per_sample);
    const int pp1 = (int)((long)(ck + 1) * pairs / chunks_per_sample);
    const int tn = p.noise_row[b], tl = p.label_row[b];

    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool upper = lane >= 32;
    const bool live_last = !HALF || !upper;
    auto live = [&](int j) { return j + 1 < NJ || live_last; };
    // input rows: normally the same rows; with CFG layer-0 sharing the cond and uncond samples read the one copy
    const resid_t* xin = p.x_in ? p.x_in : p.x;
    const size_t obase = (size_t)b * p.ntok;
    const size_t ibase = p.x_in ? (size_t)(p.src_row ? p.src_row[b] : b % p.src_batch) * p.ntok : obase;

    // Two rows per wave at a time (independent reduction chains fill the DPP wait states), with the next
    // pair's HBM loads issued before the current pair is processed (the first pair's before the table fill).
    float2 xr[2][NJ];
    bf16x2 ar[2][NJ];
    auto fetch = [&](size_t row, float2 (&xv)[NJ], bf16x2 (&av)[NJ]) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = j * 128 + 2 * lane;
            if (live(j)) {
                xv[j] = rs_load2(xin + row * d + n);
                av[j] = *reinterpret_cast<const bf16x2*>(p.att + row * d + n);
            } else {
                xv[j] = make_float2(0.f, 0.f);
                av[j] = bf16x2{(bf16)0.f, (bf16)0.f};
            }
        }
    };
    int pr = pp0 + wid;
    if (pr < pp1) {
        fetch(ibase + 2 * (size_t)pr, xr[0], ar[0]);
        fetch(ibase + 2 * (size_t)pr + 1, xr[1], ar[1]);
    }

    {
        const float4* wl = reinterpret_cast<const float4*>(p.wq + (size_t)tl * H * d);
        const float4* wn = reinterpret_cast<const float4*>(p.wq + (size_t)tn * H * d);
        float4* dst = reinterpret_cast<float4*>(wd);
        for (int i = threadIdx.x; i < H * d / 4; i += 256) {
            const float4 a = wl[i], c = wn[i];
            dst[i] = make_float4(a.x - c.x, a.y - c.y, a.z - c.z, a.w - c.w);
        }
    }
    for (int i = threadIdx.x; i < d; i += 256) {
        const float a = p.v[(size_t)tn * p.v_ld + i];
        vn[i] = a;
        vdiff[i] = p.v[(size_t)tl * p.v_ld + i] - a;
    }
    if (threadIdx.x < H) bw[threadIdx.x] = p.bwq[(size_t)tl * H + threadIdx.x] - p.bwq[(size_t)tn * H + threadIdx.x];
    __syncthreads();
    // lane's features of group j belong to head 2j + (lane >> 5)
    float bwl[NJ];
#pragma unroll
    for (int hh = 0; hh < NJ; ++hh) bwl[hh] = live(hh) ? bw[2 * hh + (upper ? 1 : 0)] : 0.f;

    for (; pr < pp1; pr += 4) {
        f32x2 v[2][NJ];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                v[u][j][0] = xr[u][j].x + (float)ar[u][j][0];        // x = SA(LN1 x) + x
                v[u][j][1] = xr[u][j].y + (float)ar[u][j][1];
            }
        const size_t row = obase + 2 * (size_t)pr;
        if (pr + 4 < pp1) {
            fetch(ibase + 2 * (size_t)(pr + 4), xr[0], ar[0]);
            fetch(ibase + 2 * (size_t)(pr + 4) + 1, xr[1], ar[1]);
        }
        if (p.sa_out) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    if (live(j)) *reinterpret_cast<f32x2*>(p.sa_out + (row + u) * d + j * 128 + 2 * lane) = v[u][j];
        }
        float mean[2], rstd[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x2 s2 = v[u][0];
#pragma unroll
            for (int j = 1; j < NJ; ++j) s2 += v[u][j];
            mean[u] = wave_sum(s2[0] + s2[1]) * inv_d;
        }
        f32x2 c[2][NJ];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x2 q2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                c[u][j] = live(j) ? v[u][j] - mean[u] : f32x2{0.f, 0.f};
                q2 = __builtin_elementwise_fma(c[u][j], c[u][j], q2);
            }
            rstd[u] = __builtin_amdgcn_rsqf(fmaf(wave_sum(q2[0] + q2[1]), inv_d, kLnEps));
        }

        // per-head logit difference -> sigmoid weight of the label token.  Packed-fp32 FMAs over the lane's
        // feature pairs; the cross-lane sums of a head PAIR share one v_permlane32_swap (lanes 0-31 finish
        // head 2hh, lanes 32-63 head 2hh+1 -- exactly the head whose features each half holds).
        float plab[2][NJ];
#pragma unroll
        for (int hh = 0; hh < NJ; ++hh) {
            f32x2 acc[2][2] = {{{0.f, 0.f}, {0.f, 0.f}}, {{0.f, 0.f}, {0.f, 0.f}}};
            const float* w0 = wd + (2 * hh) * d + 2 * lane;
            const float* w1 = w0 + d;
            const bool h1 = !HALF || hh + 1 < NJ;              // head 2 hh + 1 exists
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const f32x2 a = live(j) ? *reinterpret_cast<const f32x2*>(w0 + j * 128) : f32x2{0.f, 0.f};
                const f32x2 e = (h1 && live(j)) ? *reinterpret_cast<const f32x2*>(w1 + j * 128) : f32x2{0.f, 0.f};
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    acc[u][0] = __builtin_elementwise_fma(c[u][j], a, acc[u][0]);
                    acc[u][1] = __builtin_elementwise_fma(c[u][j], e, acc[u][1]);
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float p0 = acc[u][0][0] + acc[u][0][1], p1 = acc[u][1][0] + acc[u][1][1];
                const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(p0), __float_as_uint(p1), false, false);
                const float dl = half_sum(__uint_as_float(sw[0]) + __uint_as_float(sw[1])) * rstd[u] + bwl[hh];
                plab[u][hh] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-dl * 1.44269504088896340736f));
            }
            __builtin_amdgcn_sched_barrier(0);     // keep the next head pair's 2 x NJ LDS reads from being hoisted (VGPRs)
        }
        // x += p_noise v_n + p_label v_l ; then LN3
        float mean3[2], rstd3[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x2 s2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!live(j)) continue;
                const int n = j * 128 + 2 * lane;
                const f32x2 a = *reinterpret_cast<const f32x2*>(vn + n);
                const f32x2 dd = *reinterpret_cast<const f32x2*>(vdiff + n);
                const f32x2 pl = {plab[u][j], plab[u][j]};
                v[u][j] += __builtin_elementwise_fma(pl, dd, a);
                rs_store2(p.x + (row + u) * d + n, make_float2(v[u][j][0], v[u][j][1]));
                s2 += v[u][j];
            }
            mean3[u] = wave_sum(s2[0] + s2[1]) * inv_d;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x2 q2 = {0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                if (!live(j)) continue;
                v[u][j] -= mean3[u];
                q2 = __builtin_elementwise_fma(v[u][j], v[u][j], q2);
            }
            rstd3[u] = __builtin_amdgcn_rsqf(fmaf(wave_sum(q2[0] + q2[1]), inv_d, kLnEps));
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            if (!live(j)) continue;
            const int n = j * 128 + 2 * lane;
            const f32x2 gg = *reinterpret_cast<const f32x2*>(p.ln3_w + n);
            const f32x2 bb = *reinterpret_cast<const f32x2*>(p.ln3_b + n);
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const f32x2 r = __builtin_elementwise_fma(v[u][j] * rstd3[u], gg, bb);
                bf16x2 o;
                o[0] = (bf16)r[0];
                o[1] = (bf16)r[1];
                *reinterpret_cast<bf16x2*>(p.xn3 + (row + u) * d + n) = o;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// d % 256 == 0 (the 100 M model): lane l holds features {4l .. 4l+3} + 256 j -- 8-byte loads and stores of the bf16 streams -- and the
// per-head logit dot products run on the MATRIX pipe (round 4; up to 16 heads).
// The 4 H d fp32 MACs per row pair of the round-3 VALU kernel (cross_row_q4_kernel, lane = 4 features + 256 j; retired) were 11 of its 46 us at C1 (profiles/r03_cross_row_attribution.txt) with the
// matrix cores idle.  Here a 512-thread workgroup walks 16-row groups of one sample: every wave brings in one row pair (the next pair's
// loads in flight), forms x1 = x + att and its LayerNorm-2 statistics as before, and parks the CENTRED rows in an LDS tile [16][d] as a
// SPLIT bf16 pair (hi = bf16(c), lo = bf16(c - hi): 16 significant bits; centring first keeps rows with a large common offset exact, g9).
// After one barrier the tile's logits against the H folded query-difference vectors are v_mfma_f32_16x16x32_bf16 products
// hi.hi + lo.hi + hi.lo (fp32 accumulate: the logits keep fp32-grade accuracy, which plain bf16 operands did not: forward rel-rms
// 6.5e-3 instead of 6.3e-3 on g5) with the K range split over the eight waves: wave w multiplies features [d w / 8, d (w + 1) / 8), whose
// slices of the query-difference vectors (split the same way) it keeps in REGISTERS for the whole launch -- no table in LDS, no table fill.
// D[head][row] partials land with a lane = (row, head quad) and cross the waves through 8 KB of LDS (second barrier); every wave then sums
// the eight partials of its own two rows, applies rstd and the beta term, takes the sigmoids and finishes its rows as before.
// LDS images: 16-byte chunk c of row r at chunk c ^ r: conflict-free for the row writes (ds_write_b64) and for the MFMA operand reads (a
// ds_read_b128 lane group mixes two k-quarters of eight rows each; chunk = 4 kb + kq keeps their slots apart).
template <int NQ>
__global__ __launch_bounds__(512) void cross_row_mfma_kernel(CrossRowParams p, int groups_per_wg) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int d = NQ * 256, H = NQ * 4, PITCH = d * 2;
    constexpr float inv_d = 1.0f / (float)d;
    char* tileH = smem;                                              // [16][PITCH] bf16 hi halves of the group's centred rows
    char* tileL = tileH + 16 * PITCH;                                // [16][PITCH] lo halves
    float* part = reinterpret_cast<float*>(tileL + 16 * PITCH);      // [8 waves][16 rows][16 heads] partial logits
    float* vn = part + 8 * 256;                                      // [d] value row of the noise token
    float* vdiff = vn + d;                                           // [d] v_label - v_noise

    const int wgs_per_sample = (p.ntok >> 4) / groups_per_wg;
    const int b = blockIdx.x / wgs_per_sample;
    const int g0 = (blockIdx.x - b * wgs_per_sample) * groups_per_wg;   // first 16-row group of this workgroup inside the sample
    const int tn = p.noise_row[b], tl = p.label_row[b];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const resid_t* xin = p.x_in ? p.x_in : p.x;
    const size_t obase = (size_t)b * p.ntok;
    const size_t ibase = p.x_in ? (size_t)(p.src_row ? p.src_row[b] : b % p.src_batch) * p.ntok : obase;

    auto pair_row = [&](int g) { return 16 * (g0 + g) + 2 * wid; };   // this wave's row pair of group g (row inside the sample)
    // the next row pair's loads are in flight while the current one is processed (a second pair in flight measured 1 us SLOWER: 40.8 vs 39.7; round 4:
    // the pairs of the next TWO groups by global -> LDS DMA into per-wave slots, own-vmcnt waits, 151 registers, bitwise the same result: 42.3 vs 37.4 us --
    // bytes in flight are not what the kernel waits for, the per-group chain of reductions and its two barriers is)
    resid4_t xr[2][NQ];
    bf16x4 ar[2][NQ];
    auto fetch = [&](size_t row, resid4_t (&xv)[NQ], bf16x4 (&av)[NQ]) {
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int n = j * 256 + 4 * lane;
            xv[j] = rs_raw4(xin + row * d + n);
            av[j] = *reinterpret_cast<const bf16x4*>(p.att + row * d + n);
        }
    };
    fetch(ibase + pair_row(0), xr[0], ar[0]);
    fetch(ibase + pair_row(0) + 1, xr[1], ar[1]);

    const int tok = lane & 15, kq = lane >> 4;                       // MFMA roles: row of an operand / output column, and k-quarter / head quad
    // A operand (rows = heads), this wave's K slice, split hi / lo: K-block kb = wid NQ + s2 covers features 32 kb .. 32 kb + 31, of which this
    // lane holds 8 kq .. 8 kq + 7.  (Operand rows H .. 15 repeat the last head: their outputs are never read.)
    bf16x8 wh[NQ], wlo[NQ];
    {
        const int hrow = tok < H ? tok : H - 1;
        const float* wlp = p.wq + ((size_t)tl * H + hrow) * d;
        const float* wnp = p.wq + ((size_t)tn * H + hrow) * d;
#pragma unroll
        for (int s2 = 0; s2 < NQ; ++s2) {
            const int f = 32 * (wid * NQ + s2) + 8 * kq;
            const float4 a0 = *reinterpret_cast<const float4*>(wlp + f), a1 = *reinterpret_cast<const float4*>(wlp + f + 4);
            const float4 c0 = *reinterpret_cast<const float4*>(wnp + f), c1 = *reinterpret_cast<const float4*>(wnp + f + 4);
            const float df[8] = {a0.x - c0.x, a0.y - c0.y, a0.z - c0.z, a0.w - c0.w, a1.x - c1.x, a1.y - c1.y, a1.z - c1.z, a1.w - c1.w};
#pragma unroll
            for (int e2 = 0; e2 < 8; ++e2) {
                const bf16 hi = (bf16)df[e2];
                wh[s2][e2] = hi;
                wlo[s2][e2] = (bf16)(df[e2] - (float)hi);
            }
        }
    }
    for (int i = threadIdx.x; i < d; i += 512) {
        const float a = p.v[(size_t)tn * p.v_ld + i];
        vn[i] = a;
        vdiff[i] = p.v[(size_t)tl * p.v_ld + i] - a;
    }
    // lane's features of group j belong to head 4 j + (lane >> 4): beta contribution to that head's logit difference
    float bwl[NQ];
#pragma unroll
    for (int j = 0; j < NQ; ++j) bwl[j] = p.bwq[(size_t)tl * H + 4 * j + (lane >> 4)] - p.bwq[(size_t)tn * H + 4 * j + (lane >> 4)];
    const bool fold3 = p.ln3_stats != nullptr;

    for (int g = 0; g < groups_per_wg; ++g) {
        // ---- phase A: the wave's row pair -> x1, LayerNorm-2 statistics, centred split-bf16 rows into the tile
        f32x4 v[2][NQ];                                              // x1 = x + att, fp32
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const float4 xw = rs_widen4(xr[u][j]);
                v[u][j][0] = xw.x + (float)ar[u][j][0];              // x = SA(LN1 x) + x
                v[u][j][1] = xw.y + (float)ar[u][j][1];
                v[u][j][2] = xw.z + (float)ar[u][j][2];
                v[u][j][3] = xw.w + (float)ar[u][j][3];
            }
        if (g + 1 < groups_per_wg) {
            fetch(ibase + pair_row(g + 1), xr[0], ar[0]);
            fetch(ibase + pair_row(g + 1) + 1, xr[1], ar[1]);
        }
        const size_t row = obase + pair_row(g);
        if (p.sa_out) {
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int j = 0; j < NQ; ++j)
                    *reinterpret_cast<f32x4*>(p.sa_out + (row + u) * d + j * 256 + 4 * lane) = v[u][j];
        }
        float rstd[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 s4 = v[u][0];
#pragma unroll
            for (int j = 1; j < NQ; ++j) s4 += v[u][j];
            const float mean = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3])) * inv_d;
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
            const int gr = 2 * wid + u;                              // row inside the group's tile
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const f32x4 c = v[u][j] - mean;
                q4 = __builtin_elementwise_fma(c, c, q4);
                bf16x4 oh, ol;
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) { oh[e2] = (bf16)c[e2]; ol[e2] = (bf16)(c[e2] - (float)oh[e2]); }
                const int off = gr * PITCH + ((((32 * j + (lane >> 1)) ^ gr) << 4) | ((lane & 1) << 3));
                *reinterpret_cast<bf16x4*>(tileH + off) = oh;
                *reinterpret_cast<bf16x4*>(tileL + off) = ol;
            }
            rstd[u] = __builtin_amdgcn_rsqf(fmaf(wave_sum((q4[0] + q4[1]) + (q4[2] + q4[3])), inv_d, kLnEps));
        }
        __syncthreads();                                             // the group's 16 rows are in LDS (and nobody still reads last group's partials)
        // ---- phase B: this wave's K slice of the tile's logits on the matrix pipe, D[head 4 kq + r][row tok] partial
        {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < NQ; ++s2) {
                const int off = tok * PITCH + (((4 * (wid * NQ + s2) + kq) ^ tok) << 4);
                const bf16x8 ch = *reinterpret_cast<const bf16x8*>(tileH + off);
                const bf16x8 cl = *reinterpret_cast<const bf16x8*>(tileL + off);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[s2], ch, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[s2], cl, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wlo[s2], ch, acc, 0, 0, 0);
            }
            *reinterpret_cast<f32x4*>(part + (wid * 16 + tok) * 16 + 4 * kq) = acc;
        }
        __syncthreads();                                             // all eight K slices are in; the tile is free for the next group's rows
        // ---- phase C: logits of the wave's own two rows -> sigmoid weights; blend the two value rows, store, LayerNorm-3
        float plab[2][NQ];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const float* pp = part + (2 * wid + u) * 16 + 4 * j + (lane >> 4);
                float t = 0.f;
#pragma unroll
                for (int w2 = 0; w2 < 8; ++w2) t += pp[w2 * 256];
                const float dl = fmaf(t, rstd[u], bwl[j]);
                plab[u][j] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-dl * 1.44269504088896340736f));
                // (round 3 kept these one (row, head) at a time to save 40 registers for a 128-register build; at one workgroup per CU the 48 partial reads go together: 38.1 -> 37.6 us)
            }
        float mean3[2], rstd3[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 s4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int n = j * 256 + 4 * lane;
                const f32x4 a = *reinterpret_cast<const f32x4*>(vn + n);
                const f32x4 dd = *reinterpret_cast<const f32x4*>(vdiff + n);
                const f32x4 pl = {plab[u][j], plab[u][j], plab[u][j], plab[u][j]};
                v[u][j] += __builtin_elementwise_fma(pl, dd, a);
                rs_store4(p.x + (row + u) * d + n, make_float4(v[u][j][0], v[u][j][1], v[u][j][2], v[u][j][3]));
                if (fold3) {        // LN3 is applied by the consumer GEMM to the STORED (rounded) row: take its statistics
#pragma unroll
                    for (int e2 = 0; e2 < 4; ++e2) v[u][j][e2] = rs_round(v[u][j][e2]);
                }
                s4 += v[u][j];
            }
            mean3[u] = wave_sum((s4[0] + s4[1]) + (s4[2] + s4[3])) * inv_d;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            f32x4 q4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                v[u][j] -= mean3[u];
                q4 = __builtin_elementwise_fma(v[u][j], v[u][j], q4);
            }
            rstd3[u] = __builtin_amdgcn_rsqf(fmaf(wave_sum((q4[0] + q4[1]) + (q4[2] + q4[3])), inv_d, kLnEps));
        }
        if (fold3) {
            if (lane == 0) {
                p.ln3_stats[row] = make_float2(mean3[0], rstd3[0]);
                p.ln3_stats[row + 1] = make_float2(mean3[1], rstd3[1]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < NQ; ++j) {
                const int n = j * 256 + 4 * lane;
                const f32x4 gg = *reinterpret_cast<const f32x4*>(p.ln3_w + n);
                const f32x4 bb = *reinterpret_cast<const f32x4*>(p.ln3_b + n);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const f32x4 r = __builtin_elementwise_fma(v[u][j] * rstd3[u], gg, bb);
                    bf16x4 o;
                    o[0] = (bf16)r[0]; o[1] = (bf16)r[1]; o[2] = (bf16)r[2]; o[3] = (bf16)r[3];
                    if (p.xn3_f8) {      // fp8 GEMM mode: MX-quantise the bf16-rounded row in place of the bf16 store
                        int e8;
                        const unsigned w = mx8_pack4((float)o[0], (float)o[1], (float)o[2], (float)o[3], &e8);
                        *reinterpret_cast<unsigned*>(p.xn3_f8 + (row + u) * d + n) = w;
                        if ((lane & 7) == 0) p.xn3_s8[mx8_scale_index(n, row + u, (size_t)p.batch * p.ntok)] = (uint8_t)e8;
                    } else {
                        *reinterpret_cast<bf16x4*>(p.xn3 + (row + u) * d + n) = o;
                    }
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// out_proj + unpatchify.  16 tokens per wave, weights [pd][d] fp32 resident in LDS.
template <int NJ, bool HALF>
__global__ __launch_bounds__(256) void tail_kernel(TailParams p, int rows_per_block) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int d = NJ * 128 - (HALF ? 64 : 0);
    float* w = reinterpret_cast<float*>(smem);           // [pd][d]
    for (int i = threadIdx.x; i < p.pd * d / 4; i += 256)
        reinterpret_cast<float4*>(w)[i] = reinterpret_cast<const float4*>(p.w)[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool live_last = !HALF || lane < 32;
    auto live = [&](int j) { return j + 1 < NJ || live_last; };
    const int rows_per_wave = rows_per_block / 4;            // even
    const int total = p.batch * p.ntok;                      // even (ntok is)
    const int row_first = blockIdx.x * rows_per_block + wid * rows_per_wave;
    // two rows at a time (eight independent dot-product / reduction chains), the next pair's loads issued first
    float2 nx[2][NJ];
    auto fetch = [&](int row, float2 (&v)[NJ]) {
        const int r = row < total ? row : total - 1;
#pragma unroll
        for (int j = 0; j < NJ; ++j) v[j] = live(j) ? rs_load2(p.tok + (size_t)r * d + j * 128 + 2 * lane) : make_float2(0.f, 0.f);
    };
    fetch(row_first, nx[0]); fetch(row_first + 1, nx[1]);
    const float bias = p.b[lane < p.pd ? lane : 0];
    for (int rr = 0; rr < rows_per_wave; rr += 2) {
        const int row = row_first + rr;
        if (row >= total) return;
        float2 v[2][NJ];
#pragma unroll
        for (int u2 = 0; u2 < 2; ++u2)
#pragma unroll
            for (int j = 0; j < NJ; ++j) v[u2][j] = nx[u2][j];
        if (rr + 2 < rows_per_wave) { fetch(row + 2, nx[0]); fetch(row + 3, nx[1]); }
        float mine[2] = {0.f, 0.f};
        for (int o4 = 0; o4 < p.pd; o4 += 4) {
            float part[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = o4 + u < p.pd ? o4 + u : p.pd - 1;
                const float* wrow = w + o * d + 2 * lane;
#pragma unroll
                for (int j = 0; j < NJ; ++j) {
                    const float2 ww = live(j) ? *reinterpret_cast<const float2*>(wrow + j * 128) : make_float2(0.f, 0.f);
#pragma unroll
                    for (int u2 = 0; u2 < 2; ++u2)
                        part[u2][u] = fmaf(v[u2][j].x, ww.x, fmaf(v[u2][j].y, ww.y, part[u2][u]));
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int u2 = 0; u2 < 2; ++u2) {
                    const float tot = wave_sum(part[u2][u]);
                    if (lane == o4 + u) mine[u2] = tot + bias;
                }
        }
        if (lane < p.pd) {
            // feature f = (c, u, v) of token (ti, tj) -> out[b, c, ti*p+u, tj*p+v]
            const int c = lane / (p.p * p.p), uv = lane - c * p.p * p.p;
            const int u = uv / p.p, vv = uv - u * p.p;
#pragma unroll
            for (int u2 = 0; u2 < 2; ++u2) {
                const int r = row + u2;
                if (r < total) {
                    const int b = r / p.ntok, t = r - b * p.ntok;
                    const int ti = t / p.grid, tj = t - ti * p.grid;
                    p.out[(((size_t)b * p.C + c) * p.S + (ti * p.p + u)) * p.S + (tj * p.p + vv)] = mine[u2];
                }
            }
        }
    }
}

#ifdef TLD_RESID_BF16
// ------------------------------------------------------------------------------------------------
// Patch embedding on the matrix pipe (round 4; patch_dim == 16 -- four latent channels in 2 x 2 patches, every published model -- and
// d % 256 == 0).  embed_kernel above is one latency chain per row (readlane-broadcast taps, four wave-wide reductions): 52 us per forward
// for 16 K rows.  Here a 4-wave workgroup takes 32 token rows; every lane (token, half) builds its token's conv outputs / LayerNorm(16)
// values 8 half .. 8 half + 7 in registers -- exactly the K slice the B operand of v_mfma_f32_32x32x16_bf16 wants from it -- as a split
// bf16 pair, and Linear(16 -> d) is three MFMAs (hi.hi + hi.lo + lo.hi: fp32-grade) per 32-feature tile against the weight image in LDS;
// wave w owns feature tiles [w d / 128, (w + 1) d / 128), whose accumulators stay in registers through the two-pass LayerNorm(d) (row sums
// cross the waves through LDS).  Output rows leave as whole 128-byte segments through a per-wave transpose patch.  tld/denoiser.py:34-45,75-77.
template <int TPW>      // 32-feature tiles per wave: d = 128 TPW, TPW even
__global__ __launch_bounds__(256) void embed_mfma_kernel(EmbedParams p, const bf16* __restrict__ wl_hl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int d = TPW * 128, PD = 16, PP = 144;
    // (round 6: the Linear weight's split-bf16 rows go from L2 straight into the MFMA operand registers -- lane (l31, hi) of tile t wants the 16 bytes
    // [plane][feature 32 t + l31][8 hi .. 8 hi + 7], and a wave's 64 lanes read one contiguous KiB -- instead of being copied into a 48 KiB LDS image by every
    // 32-row workgroup first: the fill was as many bytes as the workgroup's output)
    float* cw = reinterpret_cast<float*>(smem);                   // [16][16] conv weight (row = output)
    float* red = cw + PD * PD;                                    // [3][4 waves][32 tokens] row partials (sum; centred squares; rounded sum) + [4][32] rounded squares
    float* vec = red + 4 * 4 * 32;                                // [3][d]: Linear bias, LayerNorm(d) weight and bias (read per feature quad by every token)
    char* patch = reinterpret_cast<char*>(vec + 3 * d);           // [4 waves][32 tokens][PP] output transpose
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int l31 = lane & 31, hi = lane >> 5;
    const int total = p.batch * p.ntok;
    const int grow = blockIdx.x * 32 + l31;
    const int row = grow < total ? grow : total - 1;
    const int b = row / p.ntok, tk = row - b * p.ntok;
    const int ti = tk / p.grid, tj = tk - ti * p.grid;
    // the token's 16 patch inputs, k = (c, u, v)
    float xin[PD];
    {
        const int pp = p.p * p.p;
        const float* xb = p.x + (size_t)(p.src_row ? p.src_row[b] : b % p.src_batch) * p.C * p.S * p.S;
#pragma unroll
        for (int k = 0; k < PD; ++k) {
            const int c = k / pp, uv = k - c * pp, u = uv / p.p, v = uv - u * p.p;
            xin[k] = xb[((size_t)c * p.S + (ti * p.p + u)) * p.S + (tj * p.p + v)];
        }
    }
    bf16x8 whf[TPW], wlf[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const int f = 32 * (wid * TPW + t) + l31;
        whf[t] = *reinterpret_cast<const bf16x8*>(wl_hl + (size_t)f * PD + hi * 8);
        wlf[t] = *reinterpret_cast<const bf16x8*>(wl_hl + ((size_t)d + f) * PD + hi * 8);
    }
    if (threadIdx.x < PD * PD) cw[threadIdx.x] = p.conv_w[threadIdx.x];
    for (int i = threadIdx.x; i < 3 * d / 4; i += 256) {
        const int which = i / (d / 4), j = i - which * (d / 4);
        const float* src = which == 0 ? p.lin_b : (which == 1 ? p.ln2_w : p.ln2_b);
        reinterpret_cast<float4*>(vec)[i] = reinterpret_cast<const float4*>(src)[j];
    }
    __syncthreads();
    // conv outputs o = 8 hi + e, then LayerNorm(16) over the token's 16 outputs (8 here, 8 in lane ^ 32)
    float pv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int o = 8 * hi + e;
        const float4* wr = reinterpret_cast<const float4*>(cw + o * PD);
        float a = p.conv_b[o];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) {
            const float4 w4 = wr[k4];
            a = fmaf(w4.x, xin[4 * k4], a); a = fmaf(w4.y, xin[4 * k4 + 1], a); a = fmaf(w4.z, xin[4 * k4 + 2], a); a = fmaf(w4.w, xin[4 * k4 + 3], a);
        }
        pv[e] = a;
    }
    auto pair_sum = [&](float v) {          // + the partner lane (same token, other half)
        const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
        return __uint_as_float(r[0]) + __uint_as_float(r[1]);
    };
    float s8 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s8 += pv[e];
    const float mean1 = pair_sum(s8) * (1.0f / PD);
    float q8 = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { pv[e] -= mean1; q8 = fmaf(pv[e], pv[e], q8); }
    const float rstd1 = 1.0f / sqrtf(pair_sum(q8) * (1.0f / PD) + kLnEps);
    bf16x8 bh, bl;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int o = 8 * hi + e;
        const float pn = pv[e] * rstd1 * p.ln1_w[o] + p.ln1_b[o];
        bh[e] = (bf16)pn;
        bl[e] = (bf16)(pn - (float)bh[e]);
    }
    // Linear(16 -> d): this wave's TPW feature tiles, D[feature][token]
    f32x16 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        const bf16x8 wh = whf[t], wlo = wlf[t];
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bh, z, 0, 0, 0);
        z = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bl, z, 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wlo, bh, z, 0, 0, 0);
    }
    // + bias; LayerNorm(d), two passes over the registers; the row's other features live in the partner lane and in the other three waves
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 b4 = *reinterpret_cast<const float4*>(vec + 32 * (wid * TPW + t) + 8 * q + 4 * hi);
            acc[t][4 * q + 0] += b4.x; acc[t][4 * q + 1] += b4.y; acc[t][4 * q + 2] += b4.z; acc[t][4 * q + 3] += b4.w;
            s += (acc[t][4 * q + 0] + acc[t][4 * q + 1]) + (acc[t][4 * q + 2] + acc[t][4 * q + 3]);
        }
    s = pair_sum(s);
    if (!hi) red[wid * 32 + l31] = s;
    __syncthreads();
    const float mean2 = ((red[l31] + red[32 + l31]) + (red[64 + l31] + red[96 + l31])) * (1.0f / d);
    float qq = 0.f;
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[t][r] -= mean2; qq = fmaf(acc[t][r], acc[t][r], qq); }
    qq = pair_sum(qq);
    if (!hi) red[128 + wid * 32 + l31] = qq;
    __syncthreads();
    const float rstd2 = 1.0f / sqrtf(((red[128 + l31] + red[160 + l31]) + (red[192 + l31] + red[224 + l31])) * (1.0f / d) + kLnEps);
    // affine + position table -> bf16, two tiles (64 features = 128 B per token) at a time through the wave's transpose patch
    char* T = patch + wid * 32 * PP;
    float ssum = 0.f, ssq = 0.f;
    // (the token's position-table values -- the only per-token global loads left in this loop -- are fetched one tile PAIR ahead: as loads
    // inside the loop they exposed one L2 round trip per feature quad, 24 per lane, and were most of the kernel's first version: 42.6 us)
    const float* prow = p.pos + (size_t)tk * d + 32 * wid * TPW + 4 * hi;
    float4 pnx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) pnx[i] = *reinterpret_cast<const float4*>(prow + 32 * (i >> 2) + 8 * (i & 3));
#pragma unroll
    for (int tp = 0; tp < TPW / 2; ++tp) {
        float4 pc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) pc[i] = pnx[i];
        if (tp + 1 < TPW / 2) {
#pragma unroll
            for (int i = 0; i < 8; ++i) pnx[i] = *reinterpret_cast<const float4*>(prow + 64 * (tp + 1) + 32 * (i >> 2) + 8 * (i & 3));
        }
#pragma unroll
        for (int tt = 0; tt < 2; ++tt) {
            const int t = 2 * tp + tt;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n = 32 * (wid * TPW + t) + 8 * q + 4 * hi;
                const float4 g4 = *reinterpret_cast<const float4*>(vec + d + n);
                const float4 c4 = *reinterpret_cast<const float4*>(vec + 2 * d + n);
                const float4 pe = pc[tt * 4 + q];
                bf16x4 o;
                o[0] = (bf16)(acc[t][4 * q + 0] * rstd2 * g4.x + c4.x + pe.x);
                o[1] = (bf16)(acc[t][4 * q + 1] * rstd2 * g4.y + c4.y + pe.y);
                o[2] = (bf16)(acc[t][4 * q + 2] * rstd2 * g4.z + c4.z + pe.z);
                o[3] = (bf16)(acc[t][4 * q + 3] * rstd2 * g4.w + c4.w + pe.w);
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float r = (float)o[e]; ssum += r; ssq = fmaf(r, r, ssq); }
                *reinterpret_cast<bf16x4*>(T + l31 * PP + (tt * 32 + 8 * q + 4 * hi) * 2) = o;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int r = it * 8 + (lane >> 3), ch = lane & 7;
            const u32x4 v = *reinterpret_cast<const u32x4*>(T + r * PP + ch * 16);
            const int gr = blockIdx.x * 32 + r;
            if (gr < total) *reinterpret_cast<u32x4*>(p.tok + (size_t)gr * d + 32 * (wid * TPW + 2 * tp) + ch * 8) = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (p.stats_out) {      // LayerNorm-1 statistics of block 0 (sum, sum of squares of the ROUNDED row), consumed by its QKV GEMM epilogue
        ssum = pair_sum(ssum); ssq = pair_sum(ssq);
        if (!hi) { red[256 + wid * 32 + l31] = ssum; red[384 + wid * 32 + l31] = ssq; }
        __syncthreads();
        if (wid == 0 && !hi && grow < total) {
            const float a = (red[256 + l31] + red[288 + l31]) + (red[320 + l31] + red[352 + l31]);
            const float a2 = (red[384 + l31] + red[416 + l31]) + (red[448 + l31] + red[480 + l31]);
            *reinterpret_cast<float4*>(p.stats_out + (size_t)grow * kLnSlots) = make_float4(a, a2, 0.f, 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// out_proj + unpatchify on the matrix pipe (round 4; bf16 residual stream, pd d <= 40960).  The VALU kernel above spends a wave-wide
// reduction per (row, output feature) -- 16 per row at the 100 M model -- and was a 43 us latency chain per forward for 2 MFLOP per row.
// Here D[feature][token] = W[pd x d] . x[16 tokens x d]^T per wave as d / 32 v_mfma_f32_16x16x32_bf16 steps per 16-feature tile: the token
// rows are ALREADY the operand format (bf16, feature-contiguous: lane (token, k-quarter) loads its 16 bytes straight from the residual
// stream), the weights sit in LDS as a split bf16 pair (hi + lo: fp32-grade products, same trick as cross_row's logits), accumulation fp32.
// A lane ends with 4 consecutive output features of its token: bias, then the pixel-shuffle store (tld/denoiser.py:47-52,72,82).
template <int NT>       // 16-feature tiles covering patch_dim (1 .. 4)
__global__ __launch_bounds__(256) void tail_mfma_kernel(TailParams p, const bf16* __restrict__ whl) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int d = p.d, PITCH = d * 2, pdp = NT * 16;
    char* wh = smem;                                  // [pdp][PITCH] hi halves (rows >= pd: zeros), chunk c of row r at chunk c ^ (r & 15)
    char* wl = smem + pdp * PITCH;                    // lo halves
    const int chunks = d >> 3;
    for (int i = threadIdx.x; i < 2 * pdp * chunks; i += 256) {
        const int plane = i / (pdp * chunks), rem = i - plane * pdp * chunks;
        const int r = rem / chunks, c = rem - r * chunks;
        u32x4 v = {0u, 0u, 0u, 0u};
        if (r < p.pd) v = *reinterpret_cast<const u32x4*>(whl + ((size_t)plane * p.pd + r) * d + c * 8);
        *reinterpret_cast<u32x4*>((plane ? wl : wh) + r * PITCH + ((c ^ (r & 15)) << 4)) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int tok = lane & 15, kq = lane >> 4;
    const int total = p.batch * p.ntok;
    const int row0 = (blockIdx.x * 4 + wid) * 16;
    if (row0 >= total) return;
    const int row = row0 + tok < total ? row0 + tok : total - 1;
    const bf16* xrow = p.tok + (size_t)row * d + kq * 8;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nkb = d >> 5;
    // token fragments eight K-blocks ahead of their use (the loop is one dependent MFMA chain per tile: what it must hide is the loads)
    constexpr int PF = 8;
    bf16x8 xf[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(xrow + (i < nkb ? i : 0) * 32);
    for (int kb0 = 0; kb0 < nkb; kb0 += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int kb = kb0 + i;
            if (kb >= nkb) break;
            const bf16x8 xb = xf[i];
            if (kb + PF < nkb) xf[i] = *reinterpret_cast<const bf16x8*>(xrow + (kb + PF) * 32);
            const int chunk = 4 * kb + kq;
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const int r = t * 16 + tok;
                const int off = r * PITCH + ((chunk ^ (r & 15)) << 4);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wh + off), xb, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(*reinterpret_cast<const bf16x8*>(wl + off), xb, acc[t], 0, 0, 0);
            }
        }
    }
    if (row0 + tok >= total) return;
    const int b = row / p.ntok, tk = row - b * p.ntok;
    const int ti = tk / p.grid, tj = tk - ti * p.grid;
    const int pp = p.p * p.p;
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = t * 16 + 4 * kq + r;              // feature f = (c, u, v) of token (ti, tj) -> out[b, c, ti*p+u, tj*p+v]
            if (f < p.pd) {
                const int c = f / pp, uv = f - c * pp;
                const int u = uv / p.p, vv = uv - u * p.p;
                p.out[(((size_t)b * p.C + c) * p.S + (ti * p.p + u)) * p.S + (tj * p.p + vv)] = acc[t][r] + p.b[f];
            }
        }
}

// ------------------------------------------------------------------------------------------------
// The folded tail: out_proj applied to the last block's down projection without the 768-wide row in between,
//   out[row][f] = [x2 | hid2][row] . [Wout | W'][f]^T + b'[f],   W' = Wout Wd, b' = Wout bd + bo  (tld_tail_fold_math.h),
// one skinny product over K = d + hid per token row, bound by the hid2 rows it streams from HBM.  Same MFMA roles as tail_mfma_kernel (weights = A,
// 16 token rows = B, split bf16 weights hi + lo, fp32 accumulation, the same pixel-shuffle store), but:
//   * K does not fit LDS as a split pair, so a lane takes its weight fragments from L2 into registers, and one fragment serves the RT 16-row tiles
//     of the workgroup: weight bytes per workgroup = 2 pdp / (16 RT) of the activation bytes;
//   * the K-blocks of 32 are dealt to the workgroup's 8 waves in contiguous runs of ceil(nkb / 8) and the 8 partial sums meet in LDS in the fixed
//     order ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)): the summation order is a function of d and hid alone, never of the batch or of RT -- a row's
//     result is the same bits in every launch.  Each wave runs RT x NT independent accumulator chains.
// RT follows the launch size (launch_tail): 1 for small launches -- one image, 256 rows, is 16 workgroups of 8 short chains.
template <int NT, int RT>
__global__ __launch_bounds__(512) void tail_fold_kernel(TailParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];       // [8 waves][RT x NT][64 lanes] f32x4
    f32x4* red = reinterpret_cast<f32x4*>(smem);
    const int d = p.d, K = d + p.hidn, pdp = NT * 16;
    // (wid through readfirstlane: the K-block guards below must be SCALAR branches -- as lane predicates the compiler drops the branch, and an MFMA does not
    // honour EXEC: the guarded product would be accumulated anyway)
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tok = lane & 15, kq = lane >> 4;
    const int total = p.batch * p.ntok;
    const int row0 = blockIdx.x * (RT * 16);
    const int nkb = K >> 5, dkb = d >> 5;                             // d % 64 == 0: a K-block lies in x2 or in hid2, never across
    const int per = (nkb + 7) >> 3;
    const int kb_lo = wid * per, kb_hi = kb_lo + per < nkb ? kb_lo + per : nkb;
    unsigned xoff[RT], hoff[RT];                                      // element offsets of this lane's rows (M hid 2 < 4 GiB: tld_engine_create)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = row0 + rt * 16 + tok;
        const unsigned row = (unsigned)(r < total ? r : total - 1);
        xoff[rt] = row * (unsigned)d + kq * 8; hoff[rt] = row * (unsigned)p.hidn + kq * 8;
    }
    const bf16* wbase = p.wf_hl + (size_t)tok * K + kq * 8;
    const size_t lo_plane = (size_t)pdp * K;
    f32x4 acc[RT][NT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[rt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Two register buffers of G K-blocks each: the loads of one group are all in flight while the other group's MFMAs run.  The loads are unconditional
    // (past the wave's run they repeat a valid address and the value is dropped), only the MFMAs are guarded, by a wave-uniform branch: the loop has no
    // load behind a condition, which keeps the waits counted.  G from the registers a lane can spare: the small-launch forms (RT 1) run few waves per CU
    // and need the deeper prefetch, the large-launch forms hide latency by occupancy (two workgroups per CU at <= 128 registers).
    constexpr int G = RT == 1 ? (NT == 1 ? 4 : NT == 2 ? 2 : 1) : 1;
    bf16x8 xa[2][G][RT], wh[2][G][NT], wl[2][G][NT];
    auto fetch = [&](int buf, int kb0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            int kb = kb0 + g;
            kb = kb < nkb ? kb : nkb - 1;
            const bool in_x = kb < dkb;                               // wave-uniform
            const int ko = (in_x ? kb : kb - dkb) * 32;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                xa[buf][g][rt] = *reinterpret_cast<const bf16x8*>(in_x ? p.tok + xoff[rt] + ko : p.hid + hoff[rt] + ko);
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                const bf16* w = wbase + (size_t)t * 16 * K + kb * 32;
                wh[buf][g][t] = *reinterpret_cast<const bf16x8*>(w);
                wl[buf][g][t] = *reinterpret_cast<const bf16x8*>(w + lo_plane);
            }
        }
    };
    auto mma = [&](int buf, int kb0) {                                // K-blocks in ascending order, hi then lo: the one summation order of a chain
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (kb0 + g < kb_hi) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wh[buf][g][t], xa[buf][g][rt], acc[rt][t], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < NT; ++t) acc[rt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wl[buf][g][t], xa[buf][g][rt], acc[rt][t], 0, 0, 0);
            }
        }
    };
    fetch(0, kb_lo);
    for (int kb0 = kb_lo; kb0 < kb_hi; kb0 += 2 * G) {
        fetch(1, kb0 + G);
        __builtin_amdgcn_sched_barrier(0);                            // (the loads stay ahead of the other buffer's MFMAs: sunk behind them they wait uncounted)
        mma(0, kb0);
        __builtin_amdgcn_sched_barrier(0);
        fetch(0, kb0 + 2 * G);
        __builtin_amdgcn_sched_barrier(0);
        mma(1, kb0 + G);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int t = 0; t < NT; ++t) red[(wid * (RT * NT) + rt * NT + t) * 64 + lane] = acc[rt][t];
    __syncthreads();
    const int pp = p.p * p.p;
    for (int it = wid; it < RT * NT; it += 8) {
        const int rt = it / NT, t = it - rt * NT;
        f32x4 s[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) s[w] = red[(w * (RT * NT) + it) * 64 + lane];
        const f32x4 sum = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
        const int row = row0 + rt * 16 + tok;
        if (row >= total) continue;
        const int b = row / p.ntok, tk = row - b * p.ntok;
        const int ti = tk / p.grid, tj = tk - ti * p.grid;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int f = t * 16 + 4 * kq + r;              // feature f = (c, u, v) of token (ti, tj) -> out[b, c, ti*p+u, tj*p+v]
            if (f < p.pd) {
                const int c = f / pp, uv = f - c * pp;
                const int u = uv / p.p, vv = uv - u * p.p;
                p.out[(((size_t)b * p.C + c) * p.S + (ti * p.p + u)) * p.S + (tj * p.p + vv)] = sum[r] + p.bf[f];
            }
        }
    }
}

// debug stage of the folded tail's input row (stage hook only, never on the product path): row[i][c] = x2[i][c] + row[i][c] + bias[c], row holding
// hid2 Wd^T in fp32 (an EPI_F32 GEMM) on entry -- the unrounded residual row the folded tail's result stands for
__global__ __launch_bounds__(256) void tail_fold_debug_row_kernel(float* __restrict__ row, const bf16* __restrict__ x, const float* __restrict__ bias, int64_t n, int d) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) row[i] = ((float)x[i] + row[i]) + bias[(int)(i % d)];
}
#endif

// the four normals of elements 4 quad .. 4 quad + 3 of a request's image at forward `step` (tld_sampler_noise.h): the one function behind the NOISE flavour of the
// step kernel and tld_debug_sampler_noise
__device__ __forceinline__ void sampler_noise4(uint32_t key_lo, uint32_t key_hi, uint32_t step, uint32_t quad, float n[4]) {
    philox_normals4(sampler_noise_philox(((uint64_t)key_hi << 32) | key_lo, step, quad), n);
}

// The shaped guidance update (tld_guidance_shape.h), the two device functions behind guidance_stats_kernel, the SHAPE flavour of the
// step kernel and tld_debug_guidance_shape: the update after the momentum, and the prediction under the request's weights
__device__ __forceinline__ float guidance_dbar(float c, float u, float m, float beta) {
#pragma clang fp contract(off)
    const float d = c - u;
    return beta != 0.0f ? d + beta * m : d;
}
__device__ __forceinline__ float guidance_shaped_x0(float P, float Q, float c, float dbar) {
#pragma clang fp contract(off)
    return __builtin_fmaf(P, c, Q * dbar);
}

// One workgroup of 256 threads per request still running: no atomics, no partial sums in memory, no second pass.  Thread t owns quads t, t + 256, ...
// of the request's image, in that order, and within a quad its elements in order; it forms dbar as the step kernel will and adds to five double sums.
// The workgroup's 256 partial sums meet in LDS in a fixed halving tree (128, 64, ..., 1), and thread 0 runs guidance_shape_finalize.  The order of
// every addition depends on img alone: a request's sums, P and Q do not depend on the other requests or on where it stands in the call.  V = 4 reads a
// quad as one 16-byte load per operand; V = 1 reads the same elements in the same order one by one (img no multiple of 4, or an operand not 16-byte
// aligned) and gives the same bits.  Products of two fp32 values are exact in double, so only the additions round.
template <int V>
__global__ __launch_bounds__(256) void guidance_stats_kernel(GuidanceStatsParams p) {
#pragma clang fp contract(off)
    const int b = blockIdx.x, t = threadIdx.x;
    const GuidanceShape h = p.shape_rows[b * p.row_stride];
    const SamplerStepRow q = p.rows[b * p.row_stride];
    const int slot = (q.final_step >> 1) - 1;
    // (the whole workgroup, before any barrier.  g == 1.0f: the forward is unguided -- x0 = cond and the momentum stays, whether or not the engine
    // skipped its unconditional sample)
    if (h.neutral() || slot < 0 || q.g == 1.0f) return;
    const float* c = p.cond + (size_t)b * p.img;
    const float* u = p.unc_base + (size_t)slot * p.img;
    const bool mom = h.beta != 0.0f;
    const float* m = mom ? p.mom + (size_t)b * p.img : nullptr;
    double acc[GS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const int quads = (p.img + 3) >> 2;
    for (int qd = t; qd < quads; qd += 256) {
        const int e0 = 4 * qd;
        float cv[4], uv[4], mv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        int cnt = 4;
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(cv) = *reinterpret_cast<const float4*>(c + e0);
            *reinterpret_cast<float4*>(uv) = *reinterpret_cast<const float4*>(u + e0);
            if (mom) *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m + e0);
        } else {
            cnt = p.img - e0 < 4 ? p.img - e0 : 4;
            for (int k = 0; k < cnt; ++k) {
                cv[k] = c[e0 + k];
                uv[k] = u[e0 + k];
                if (mom) mv[k] = m[e0 + k];
            }
        }
        for (int k = 0; k < cnt; ++k) {
            const double cd = (double)cv[k], dd = (double)guidance_dbar(cv[k], uv[k], mv[k], h.beta);
            acc[GS_SC] = acc[GS_SC] + cd;
            acc[GS_SD] = acc[GS_SD] + dd;
            acc[GS_SCC] = acc[GS_SCC] + cd * cd;
            acc[GS_SDC] = acc[GS_SDC] + dd * cd;
            acc[GS_SDD] = acc[GS_SDD] + dd * dd;
        }
    }
    __shared__ double red[GS_SUMS][256];
#pragma unroll
    for (int j = 0; j < GS_SUMS; ++j) red[j][t] = acc[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
#pragma unroll
            for (int j = 0; j < GS_SUMS; ++j) red[j][t] = red[j][t] + red[j][t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        double sums[GS_SUMS];
#pragma unroll
        for (int j = 0; j < GS_SUMS; ++j) { sums[j] = red[j][0]; p.sums[(size_t)b * GS_SUMS + j] = sums[j]; }
        const GuidanceWeights w = guidance_shape_finalize(sums, p.img, q.g, h);
        p.pq[b] = make_float2(w.P, w.Q);
    }
}

// tld_debug_guidance_shape: element by element what the SHAPE flavour of the step kernel computes for x0 and stores to the momentum buffer
__global__ __launch_bounds__(256) void guidance_shape_debug_kernel(const float* __restrict__ cond, const float* __restrict__ unc, float* __restrict__ mom,
                                                                   const SamplerStepRow* __restrict__ rows, const GuidanceShape* __restrict__ shape_rows,
                                                                   const float2* __restrict__ pq, int batch, int img, float* __restrict__ x0) {
#pragma clang fp contract(off)
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)batch * img) return;
    const int b = (int)(i / img);
    const GuidanceShape h = shape_rows[b];
    const float c = cond[i], u = unc[i];
    if (h.neutral() || rows[b].g == 1.0f) { x0[i] = __builtin_fmaf(rows[b].g, c, (1.0f - rows[b].g) * u); return; }
    const bool keep = h.beta != 0.0f && mom != nullptr;
    const float db = guidance_dbar(c, u, keep ? mom[i] : 0.0f, keep ? h.beta : 0.0f);
    const float2 w = pq[b];
    x0[i] = guidance_shaped_x0(w.x, w.y, c, db);
    if (keep) mom[i] = db;
}

// ------------------------------------------------------------------------------------------------
// The sampler's elementwise step, one launch per step for all three sampler entries: CFG combine, DPM-Solver++(2M)/DDIM update,
// latent shifts, and with MASK the inpainting blend.  Sample b takes {g, a, b, c, c1, c2, s_next, final} from rows[b * row_stride]: a row per
// request (tld_sample_requests), or one row for the whole batch.  The launch covers the `active` requests still running at this step; the
// unconditional operand of sample b sits `active` samples after its conditional one.  A thread owns V consecutive elements (V = 4: one 16-byte
// access per stream; they share a sample, a channel and a mask quad because img % 4 == 0 and chan_stride % 4 == 0).  Which products the compiler
// fuses depends on how it vectorises a kernel, so contraction is off and the roundings are spelled out:
//   x0 = fma(g, cond, (1 - g) unc)      D = fma(c1, x0, -(c2 x0_prev))      x_t = (a D + b x_t) / c   with both products rounded
// MASK adds, in the same launch:
//   after the update   x_t <- m x_t + (1 - m) (s_next eps + (1 - s_next) z0)     the known region rides the forward process of the same eps
//   on the final step  x0  <- m x0  + (1 - m) z0                                  before the latent shifts
// x0_prev and trace_x0 keep the unblended prediction.  The blend is written m a + (1 - m) b: m = 1 gives a and m = 0 gives b exactly, and with
// no contraction it rounds as the fp32 reference loop does.
// SLOT (tld_sample_requests_guided): a request has an unconditional sample only at the steps it is guided at.  Its row's `final_step` then holds
// final | (slot + 1) << 1: the unconditional operand sits at sample active + slot of the model output, and a row without a slot takes x0 = cond itself.
// NOISE (tld_sample_requests_stochastic): after the update and before the blend, x_t <- x_t + e z with the product rounded, then the sum;
// e and the key come from noise_rows[b * row_stride], z from the counter (quad of the element inside the request's own image, noise_step) under that key
// (sampler_noise4).  A row with e == 0.0f draws nothing and adds nothing: the arithmetic above exactly.  The final step returns before it.
// SHAPE (tld_sample_requests_shaped), on top of SLOT and NOISE: a request whose shape row is not neutral and which has an unconditional
// slot at this step and a guidance other than 1.0f takes x0 = fma(P, cond, Q dbar), dbar = cond - unc (+ beta m), with (P, Q) from this step's guidance_stats_kernel launch, and where
// beta != 0 an inner step stores m <- dbar.  Every other request takes `combine` as it stands and touches neither table nor buffer.
// SESS (tld_session_step), on top of SLOT: the step's model output is compact (request b of the step's live set at b img, its
// unconditional sample at (active + slot) img) while x_t, x0_prev and out_latent are the session's slot-major buffers, read and written at
// req_slot[b] img; and a request's forward index -- the step of its noise counter -- comes from its noise row's `reserved`, since every live request sits at its own level.
// The arithmetic is the code above and below, untouched.
template <bool MASK, int V, bool SLOT = false, bool NOISE = false, bool SHAPE = false, bool SESS = false>
__global__ __launch_bounds__(256) void sampler_step_kernel(SamplerStepParams p) {
#pragma clang fp contract(off)
    const int i = (blockIdx.x * 256 + threadIdx.x) * V;
    const int n = p.active * p.img;
    if (i >= n) return;
    float cond[V], unc[V], prev[V], xin[V], eps[V], z[V], m[V], x0o[V], xto[V];
    auto load = [&](float* dst, const float* src) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        else dst[0] = src[0];
    };
    auto store = [&](float* dst, const float* src) {
        if constexpr (V == 4) *reinterpret_cast<float4*>(dst) = *reinterpret_cast<const float4*>(src);
        else dst[0] = src[0];
    };
    const int b = i / p.img, r = i - b * p.img;
    const int ch = r / p.chan_stride;
    const SamplerStepRow q = p.rows[b * p.row_stride];
    load(cond, p.x0_2b + i);
    const size_t si = SESS ? (size_t)p.req_slot[b] * p.img + r : (size_t)i;      // where the sample's state lives
    const int slot = SLOT ? (q.final_step >> 1) - 1 : 0;
    const bool final_step = SLOT ? (q.final_step & 1) != 0 : q.final_step != 0;
    if constexpr (SLOT) {
        if (slot >= 0) load(unc, p.x0_2b + (size_t)(p.active + slot) * p.img + r);
    } else {
        load(unc, p.x0_2b + n + i);
    }
    auto combine = [&](float c, float u) {                                    // diffusion.py:124-125
        if constexpr (SLOT) { if (slot < 0) return c; }
        return __builtin_fmaf(q.g, c, (1.0f - q.g) * u);
    };
    bool shaped = false;
    float sP = 0.0f, sQ = 0.0f, sbeta = 0.0f, mom[V], dbo[V];
#pragma unroll
    for (int v = 0; v < V; ++v) mom[v] = 0.0f;
    if constexpr (SHAPE) {
        const GuidanceShape h = p.shape_rows[b * p.row_stride];
        if (slot >= 0 && !h.neutral() && q.g != 1.0f) {
            const float2 w = p.shape_pq[b];
            shaped = true; sP = w.x; sQ = w.y; sbeta = h.beta;
            if (sbeta != 0.0f) load(mom, p.shape_mom + i);
        }
    }
    auto predict = [&](int v) {
        if constexpr (SHAPE) {
            if (shaped) {
                dbo[v] = guidance_dbar(cond[v], unc[v], mom[v], sbeta);
                return guidance_shaped_x0(sP, sQ, cond[v], dbo[v]);
            }
        }
        return combine(cond[v], unc[v]);
    };
    if constexpr (MASK) {
        load(m, p.mask + (size_t)b * p.chan_stride + (r - ch * p.chan_stride));
        load(z, p.z0 + i);
    }
    if (final_step) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            float x0 = predict(v);
            if constexpr (MASK) x0 = m[v] * x0 + (1.0f - m[v]) * z[v];
            if (ch == 3) x0 += p.sharp;                                   // diffusion.py:88
            if (ch == 0) x0 += p.bright;                                  // diffusion.py:89
            x0o[v] = x0;
        }
        store(p.out_latent + si, x0o);
        return;
    }
    load(prev, p.x0_prev + si);
    load(xin, p.x_t + si);
    if constexpr (MASK) load(eps, p.noise + i);
    float en = 0.0f, nz[V];
    if constexpr (NOISE) {
        const SamplerNoiseRow nq = p.noise_rows[b * p.row_stride];
        en = nq.e;
        if (en != 0.0f) {
            float n4[4];
            sampler_noise4(nq.key_lo, nq.key_hi, SESS ? nq.reserved : p.noise_step, (uint32_t)r >> 2, n4);
            if constexpr (V == 4) {
#pragma unroll
                for (int v = 0; v < 4; ++v) nz[v] = n4[v];
            } else {                                                          // the quad's counter, this thread's own element
                const int k = r & 3;
                nz[0] = (k & 2) ? ((k & 1) ? n4[3] : n4[2]) : ((k & 1) ? n4[1] : n4[0]);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float x0 = predict(v);
        const float D = __builtin_fmaf(q.c1, x0, -(q.c2 * prev[v]));      // diffusion.py:76 (c1=1,c2=0: :72/:79)
        float xt = (q.a * D + q.b * xin[v]) / q.c;                        // diffusion.py:81
        if constexpr (NOISE) { if (en != 0.0f) xt = xt + en * nz[v]; }
        if constexpr (MASK) {
            const float known = q.s_next * eps[v] + (1.0f - q.s_next) * z[v];
            xt = m[v] * xt + (1.0f - m[v]) * known;
        }
        x0o[v] = x0;
        xto[v] = xt;
    }
    if (p.trace_x0) store(p.trace_x0 + i, x0o);
    store(p.x_t + si, xto);
    store(p.x0_prev + si, x0o);
    if (p.trace_xt) store(p.trace_xt + i, xto);
    if constexpr (SHAPE) { if (shaped && sbeta != 0.0f) store(p.shape_mom + i, dbo); }
}

// x_start = s0 eps + (1 - s0) z0: the forward process at the first remaining level (tld/train.py:130), s0 read per sample from s0v[sample * s0_stride];
// a sample whose s0 is exactly 1 starts from eps itself and is copied
template <int V>
__global__ __launch_bounds__(256) void start_mix_kernel(const float* __restrict__ noise, const float* __restrict__ z0, const float* __restrict__ s0v,
                                                        int s0_stride, float* __restrict__ x_t, int n, int img) {
#pragma clang fp contract(off)
    const int i = (blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;
    const float s0 = s0v[(i / img) * s0_stride];
    if constexpr (V == 4) {
        const float4 e = *reinterpret_cast<const float4*>(noise + i);
        if (s0 == 1.0f) { *reinterpret_cast<float4*>(x_t + i) = e; return; }
        const float4 z = *reinterpret_cast<const float4*>(z0 + i);
        const float t = 1.0f - s0;
        *reinterpret_cast<float4*>(x_t + i) = make_float4(s0 * e.x + t * z.x, s0 * e.y + t * z.y, s0 * e.z + t * z.z, s0 * e.w + t * z.w);
    } else {
        x_t[i] = s0 == 1.0f ? noise[i] : s0 * noise[i] + (1.0f - s0) * z0[i];
    }
}

// tld_debug_sampler_noise: z[b, 4 quad + k] = element k of sampler_noise4(keys[b], steps[b], quad); a thread owns one quad, scalar stores (img need
// not be a multiple of 4: the last quad of an image is cut)
__global__ __launch_bounds__(256) void sampler_noise_debug_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ steps, int batch, int img,
                                                                  float* __restrict__ z) {
    const int quads = (img + 3) >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)batch * quads) return;
    const int b = (int)(t / quads), quad = (int)(t - (int64_t)b * quads);
    const uint64_t key = keys[b];
    float n4[4];
    sampler_noise4((uint32_t)key, (uint32_t)(key >> 32), steps[b], (uint32_t)quad, n4);
    float* dst = z + (int64_t)b * img + 4 * quad;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * quad + k < img) dst[k] = n4[k];
}

// ------------------------------------------------------------------------------------------------
// Depthwise 3x3 + bias + exact GELU.  One workgroup = one sample x 64 channels: the whole g x g image
// slab (g*g tokens x 128 B) is pulled into LDS once with 16-B coalesced loads, so HBM/L2 see every input
// exactly once (the register-window version re-read each row three times through L2).  Thread (row i,
// channel quad) then slides a 3x3 fp32 window along j: 3 ds_read_b64 + 36 FMAs + 4 GELUs + one 8-B
// store per position; weights stay in registers.  GELU uses the Abramowitz-Stegun erf (1.5e-7).
constexpr int DW_CB = kDwChannels;              // channels per workgroup (tld_launch_plan.h: the launch's grid counts them)
__global__ __launch_bounds__(256) void dwconv_gelu_kernel(const bf16* __restrict__ in, bf16* __restrict__ out,
                                                          const float* __restrict__ w9c,
                                                          const float* __restrict__ bias, int batch,
                                                          int g, int C) {
    extern __shared__ __attribute__((aligned(16))) char smem[];    // [g*g tokens][64 ch] bf16
    const int nchunk = C / DW_CB;
    const int b = blockIdx.x / nchunk, cc = blockIdx.x - b * nchunk;
    const int ntok = g * g;
    const bf16* src = in + (size_t)b * ntok * C + cc * DW_CB;
    for (int idx = threadIdx.x; idx < ntok * 8; idx += 256) {       // 8 x 16-B pieces per token
        const int t = idx >> 3, q = idx & 7;
        *reinterpret_cast<uint4*>(smem + t * 128 + q * 16) =
            *reinterpret_cast<const uint4*>(src + (size_t)t * C + q * 8);
    }
    const int cq = threadIdx.x & 15;             // channel quad within the 64-channel slab
    const int c0 = cc * DW_CB + cq * 4;
    float4 w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = *reinterpret_cast<const float4*>(w9c + (size_t)k * C + c0);
    const float4 bs = *reinterpret_cast<const float4*>(bias + c0);
    __syncthreads();

    for (int i = threadIdx.x >> 4; i < g; i += 16) {
        const bool up_ok = i > 0, dn_ok = i + 1 < g;
        auto load_col = [&](int j, float4 (&col)[3]) {
            const bool jok = j >= 0 && j < g;
#pragma unroll
            for (int du = 0; du < 3; ++du) {
                const bool ok = jok && (du == 1 || (du == 0 ? up_ok : dn_ok));
                if (ok) {
                    const bf16x4 v = *reinterpret_cast<const bf16x4*>(smem + ((i + du - 1) * g + j) * 128 + cq * 8);
                    col[du] = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
                } else {
                    col[du] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        };
        bf16* dst = out + ((size_t)b * ntok + (size_t)i * g) * C + c0;
        // one output position from the three window columns (L = j-1, M = j, R = j+1); three independent
        // accumulation chains (one per image row) keep the packed-FMA pipeline free of dependency stalls
        auto emit = [&](const float4 (&L)[3], const float4 (&Mc)[3], const float4 (&R)[3], int j) {
            float4 part[3];
#pragma unroll
            for (int du = 0; du < 3; ++du) {
                const float4 w0 = w[du * 3 + 0], w1 = w[du * 3 + 1], w2 = w[du * 3 + 2];
                part[du].x = fmaf(w2.x, R[du].x, fmaf(w1.x, Mc[du].x, w0.x * L[du].x));
                part[du].y = fmaf(w2.y, R[du].y, fmaf(w1.y, Mc[du].y, w0.y * L[du].y));
                part[du].z = fmaf(w2.z, R[du].z, fmaf(w1.z, Mc[du].z, w0.z * L[du].z));
                part[du].w = fmaf(w2.w, R[du].w, fmaf(w1.w, Mc[du].w, w0.w * L[du].w));
            }
            const float ax = (part[0].x + part[1].x) + (part[2].x + bs.x);
            const float ay = (part[0].y + part[1].y) + (part[2].y + bs.y);
            const float az = (part[0].z + part[1].z) + (part[2].z + bs.z);
            const float aw = (part[0].w + part[1].w) + (part[2].w + bs.w);
            bf16x4 o;
            o[0] = (bf16)TLD_DW_GELU(ax); o[1] = (bf16)TLD_DW_GELU(ay);
            o[2] = (bf16)TLD_DW_GELU(az); o[3] = (bf16)TLD_DW_GELU(aw);
            *reinterpret_cast<bf16x4*>(dst + (size_t)j * C) = o;
        };
        // the window rotates through three named column buffers, so no register copies are needed
        float4 c0v[3], c1v[3], c2v[3];
        load_col(-1, c0v);
        load_col(0, c1v);
        int j = 0;
        for (; j + 3 <= g; j += 3) {
            load_col(j + 1, c2v); emit(c0v, c1v, c2v, j);
            load_col(j + 2, c0v); emit(c1v, c2v, c0v, j + 1);
            load_col(j + 3, c1v); emit(c2v, c0v, c1v, j + 2);
        }
        if (j < g) { load_col(j + 1, c2v); emit(c0v, c1v, c2v, j); ++j; }
        if (j < g) { load_col(j + 1, c0v); emit(c1v, c2v, c0v, j); }
    }
}

// Same computation for grids larger than 16x16 (512 / 1024 px latents): one workgroup = one sample x 64 channels x one
// 16x16 spatial tile.  The tile plus a one-token halo (18 x 18 tokens x 128 B) is brought into LDS by direct
// global->LDS DMA (41 pieces of 8 tokens, all in flight at once; the register-staged fill it replaces waited for
// one load per iteration and the kernel ran at 2.7 TB/s).  Halo tokens outside the image are DMA'd from a clamped
// (valid) address and never contribute: rows above / below the image meet zeroed copies of the top / bottom taps,
// columns left / right of it are replaced by zero registers -- no zero fill, no predicated code in the window loop.
template <bool F8OUT>
__global__ __launch_bounds__(256) void dwconv_gelu_tiled_kernel(const bf16* __restrict__ in, bf16* __restrict__ out,
                                                                const float* __restrict__ w9c,
                                                                const float* __restrict__ bias, int batch,
                                                                int g, int C, uint8_t* __restrict__ out8,
                                                                uint8_t* __restrict__ scale8) {
    constexpr int T = 16, TP = T + 2;
    constexpr int PIECES = (TP * TP + 7) / 8;              // 1-KiB DMA pieces (8 tokens x 128 B)
    __shared__ __attribute__((aligned(16))) char tile[PIECES * 1024];
    const int nchunk = C / DW_CB;
    const int tiles = (g + T - 1) / T;
    int bid = blockIdx.x;
    const int cc = bid % nchunk; bid /= nchunk;
    const int tx = bid % tiles; bid /= tiles;
    const int ty = bid % tiles;
    const int b = bid / tiles;
    const int i0 = ty * T - 1, j0 = tx * T - 1;
    const bf16* src = in + (size_t)b * g * g * C + cc * DW_CB;
    {
        typedef const __attribute__((address_space(1))) void* gp_t;
        typedef __attribute__((address_space(3))) void* lp_t;
        const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        for (int pc = wid; pc < PIECES; pc += 4) {
            int t = pc * 8 + (lane >> 3);
            t = t < TP * TP ? t : TP * TP - 1;
            const int li = t / TP, lj = t - li * TP;
            int gi = i0 + li, gj = j0 + lj;
            gi = gi < 0 ? 0 : (gi >= g ? g - 1 : gi);
            gj = gj < 0 ? 0 : (gj >= g ? g - 1 : gj);
            const bf16* sp = src + ((size_t)gi * g + gj) * C + (lane & 7) * 8;
            __builtin_amdgcn_global_load_lds((gp_t)sp, (lp_t)(tile + pc * 1024), 16, 0, 0);
        }
    }
    const int cq = threadIdx.x & 15;
    const int c0 = cc * DW_CB + cq * 4;
    // packed-fp32 arithmetic: channel pairs {c0, c0+1} and {c0+2, c0+3} ride in f32x2 registers.  w9c / bias are the
    // HALVED tables (the conv delivers y = x / 2 and the GELU is evaluated in its half-argument form, see tld_common.h)
    f32x2 w[9][2], bs[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(w9c + (size_t)k * C + c0);
        w[k][0] = f32x2{t.x, t.y}; w[k][1] = f32x2{t.z, t.w};
    }
    {
        const float4 t = *reinterpret_cast<const float4*>(bias + c0);
        bs[0] = f32x2{t.x, t.y}; bs[1] = f32x2{t.z, t.w};
    }
    const int li = threadIdx.x >> 4;                       // output row inside the tile (0..15)
    const int gi = ty * T + li;
    {   // image rows -1 and g: zero the taps that would meet them (the halo row holds a clamped copy)
        const float mu = gi > 0 ? 1.0f : 0.0f, md = gi + 1 < g ? 1.0f : 0.0f;
#pragma unroll
        for (int t3 = 0; t3 < 3; ++t3)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) { w[t3][h2] *= mu; w[6 + t3][h2] *= md; }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // own DMA pieces landed ...
    __syncthreads();                                       // ... everybody's
    if (gi >= g) return;
    auto col = [&](int lj, f32x2 (&c)[3][2]) {             // lj: halo-tile column index 0..17
        // image columns >= g are zero padding, not the clamped copy the halo holds: the last tile of a grid that is not a multiple of 16 wide
        // (24, 40 ...) is partial, and its right edge lies inside the tile
        if (j0 + lj >= g) {
#pragma unroll
            for (int du = 0; du < 3; ++du) { c[du][0] = f32x2{0.f, 0.f}; c[du][1] = f32x2{0.f, 0.f}; }
            return;
        }
#pragma unroll
        for (int du = 0; du < 3; ++du) {
            const bf16x4 v = *reinterpret_cast<const bf16x4*>(tile + ((li + du) * TP + lj) * 128 + cq * 8);
            c[du][0] = f32x2{(float)v[0], (float)v[1]};
            c[du][1] = f32x2{(float)v[2], (float)v[3]};
        }
    };
    bf16* dst = out + ((size_t)b * g * g + (size_t)gi * g + (size_t)tx * T) * C + c0;
    const int ncols = g - tx * T < T ? g - tx * T : T;     // (8 in the last tile of a 24- or 40-wide grid)
    auto emit = [&](const f32x2 (&L)[3][2], const f32x2 (&Mc)[3][2], const f32x2 (&R)[3][2], int lj) {
        f32x2 a[2] = {bs[0], bs[1]};
#pragma unroll
        for (int du = 0; du < 3; ++du)
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2) {
                a[h2] = __builtin_elementwise_fma(w[du * 3 + 0][h2], L[du][h2], a[h2]);
                a[h2] = __builtin_elementwise_fma(w[du * 3 + 1][h2], Mc[du][h2], a[h2]);
                a[h2] = __builtin_elementwise_fma(w[du * 3 + 2][h2], R[du][h2], a[h2]);
            }
        a[0] = gelu_erf_fast2_half(a[0]); a[1] = gelu_erf_fast2_half(a[1]);
        bf16x4 o;
        o[0] = (bf16)a[0][0]; o[1] = (bf16)a[0][1]; o[2] = (bf16)a[1][0]; o[3] = (bf16)a[1][1];
        if constexpr (F8OUT) {      // fp8 GEMM mode: MX-quantise the bf16-rounded quad (8 adjacent channel quads = one 32-block)
            int e8;
            const unsigned w = mx8_pack4((float)o[0], (float)o[1], (float)o[2], (float)o[3], &e8);
            const size_t row = (size_t)b * g * g + (size_t)gi * g + (size_t)tx * T + lj;
            if (lj < ncols) {
                *reinterpret_cast<unsigned*>(out8 + row * C + c0) = w;
                if ((cq & 7) == 0) scale8[mx8_scale_index(c0, row, (size_t)batch * g * g)] = (uint8_t)e8;
            }
        } else {
            if (lj < ncols) *reinterpret_cast<bf16x4*>(dst + (size_t)lj * C) = o;
        }
    };
    auto zero = [&](f32x2 (&c)[3][2]) {
#pragma unroll
        for (int du = 0; du < 3; ++du) { c[du][0] = f32x2{0.f, 0.f}; c[du][1] = f32x2{0.f, 0.f}; }
    };
    // the window rotates through three named column buffers (no register copies); 16 = 5 x 3 + 1 positions
    f32x2 c0v[3][2], c1v[3][2], c2v[3][2];
    if (tx == 0) zero(c0v); else col(0, c0v);              // image column -1
    col(1, c1v);
    int lj = 0;
    for (; lj + 3 <= T; lj += 3) {
        col(lj + 2, c2v); emit(c0v, c1v, c2v, lj);
        col(lj + 3, c0v); emit(c1v, c2v, c0v, lj + 1);
        col(lj + 4, c1v); emit(c2v, c0v, c1v, lj + 2);
    }
    if (tx * T + T >= g) zero(c2v); else col(lj + 2, c2v);  // image column g
    emit(c0v, c1v, c2v, lj);                                // lj == 15
}

}  // namespace

// d = 64 k (k = 1 .. 16): NJ = ceil(d / 128) feature groups per lane, HALF when the last one holds 64 features
#define TLD_DISPATCH_NJ_(nj, HF, ...)                                                               \
    switch (nj) {                                                                                    \
        case 1: { constexpr int NJ = 1; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 2: { constexpr int NJ = 2; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 3: { constexpr int NJ = 3; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 4: { constexpr int NJ = 4; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 5: { constexpr int NJ = 5; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 6: { constexpr int NJ = 6; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 7: { constexpr int NJ = 7; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        case 8: { constexpr int NJ = 8; constexpr bool HALF = HF; __VA_ARGS__; } break;                    \
        default: break;                                                                              \
    }
#define TLD_DISPATCH_D(dd, ...)                                                                      \
    do {                                                                                             \
        if ((dd) % 128) TLD_DISPATCH_NJ_(((dd) + 127) / 128, true, __VA_ARGS__) else TLD_DISPATCH_NJ_((dd) / 128, false, __VA_ARGS__)  \
    } while (0)

// dynamic LDS above the 64-KiB default needs an opt-in per kernel and device (embed / out-proj / cross-attention tables at d = 1024)
#define TLD_LDS_OPT_IN(KERNEL, bytes)                                                                \
    do {                                                                                             \
        static PerDeviceMax optin;                                                                   \
        if ((bytes) > 64 * 1024)                                                                     \
            optin.run((bytes), [&] { hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (bytes)); }); \
    } while (0)

// The launchers below: make the plan (tld_launch_plan.h: every size-dependent decision), note its paths, switch on its form, launch.
void launch_embed(const EmbedParams& p, hipStream_t s) {
    const EmbedPlan e = plan_embed(p.batch, p.ntok, p.pd, p.C * p.p * p.p, p.d, p.lin_w_hl != nullptr);
    const dim3 grid(e.gx), block(e.block);
    note_paths(e.paths);
#ifdef TLD_RESID_BF16
    if (e.form == EMBED_MFMA) {
#define TLD_EM(TPW) do { TLD_LDS_OPT_IN((embed_mfma_kernel<TPW>), e.lds); hipLaunchKernelGGL((embed_mfma_kernel<TPW>), grid, block, e.lds, s, p, p.lin_w_hl); } while (0)
        switch (e.tpw) { case 2: TLD_EM(2); break; case 4: TLD_EM(4); break; case 6: TLD_EM(6); break; default: TLD_EM(8); break; }
#undef TLD_EM
        return;
    }
#endif
    TLD_DISPATCH_D(p.d, { TLD_LDS_OPT_IN((embed_kernel<NJ, HALF>), e.lds); hipLaunchKernelGGL((embed_kernel<NJ, HALF>), grid, block, e.lds, s, p); });
}

void launch_layernorm_bf16(const resid_t* x, const float* g, const float* b, bf16* out, int M, int d,
                           hipStream_t s) {
    const LayerNormPlan n = plan_layernorm(M, d, false);
    const dim3 grid(n.gx), block(n.block);
    note_paths(n.paths);
#define TLD_LNQ(NQ) hipLaunchKernelGGL(layernorm_bf16_q4_kernel<NQ>, grid, block, 0, s, x, g, b, out, M, d)
    if (n.form == LN_Q4) switch (n.nq) { case 1: TLD_LNQ(1); break; case 2: TLD_LNQ(2); break; case 3: TLD_LNQ(3); break; default: TLD_LNQ(4); break; }
    else TLD_DISPATCH_D(d, hipLaunchKernelGGL((layernorm_bf16_kernel<NJ, HALF>), grid, block, 0, s, x, g, b, out, M, d));
#undef TLD_LNQ
}

void launch_layernorm_mx8(const resid_t* x, const float* g, const float* b, uint8_t* out8, uint8_t* scale8, int M, int d,
                          hipStream_t s) {
    const LayerNormPlan n = plan_layernorm(M, d, true);
    const dim3 grid(n.gx), block(n.block);
    note_paths(n.paths);
    if (n.form != LN_MX8) return;      // LN_NONE: no such kernel at this width (unreachable: the engine's mode asks layernorm_mx8_supported first)
#define TLD_LN8(NQ) hipLaunchKernelGGL(layernorm_mx8_kernel<NQ>, grid, block, 0, s, x, g, b, out8, scale8, M, d)
    switch (n.nq) { case 1: TLD_LN8(1); break; case 2: TLD_LN8(2); break; default: TLD_LN8(3); break; }
#undef TLD_LN8
}

void launch_cross_row(const CrossRowParams& p, hipStream_t s) {
    const CrossRowPlan c = plan_cross_row(p.batch, p.ntok, p.d, p.heads, p.x_in != nullptr, p.xn3_f8 != nullptr, device_cu_count());
    const dim3 grid(c.gx), block(c.block);
    note_paths(c.paths);
    if (c.form == CROSS_MFMA) {
#define TLD_CRM(NQ) do { TLD_LDS_OPT_IN((cross_row_mfma_kernel<NQ>), c.lds); hipLaunchKernelGGL((cross_row_mfma_kernel<NQ>), grid, block, c.lds, s, p, c.gpw); } while (0)
        switch (c.nq) { case 1: TLD_CRM(1); break; case 2: TLD_CRM(2); break; case 3: TLD_CRM(3); break; default: TLD_CRM(4); break; }
#undef TLD_CRM
        return;
    }
    TLD_DISPATCH_D(p.d, { TLD_LDS_OPT_IN((cross_row_kernel<NJ, HALF>), c.lds); hipLaunchKernelGGL((cross_row_kernel<NJ, HALF>), grid, block, c.lds, s, p, c.cps); });
}

// ------------------------------------------------------------------------------------------------
// Low-latency class (round 5): the down projection of a SMALL batch as split-K -- `nsplit` fp32 slices from the persistent GEMM -- finished here:
//   x[row] = bf16(x[row] + bias + slice_0[row] + ... + slice_{nsplit-1}[row])     (fixed order)   tld/transformer_blocks.py:104,138
// plus the LayerNorm-1 partial sums (sum, sum of squares of the ROUNDED row per 96-column group) the next block's fused QKV kernel reads --
// what EPI_BIAS_RESID does in its own epilogue.  One wave per row, lane l owns columns [CPL l, CPL (l + 1)): a group is 96 / CPL adjacent lanes.
template <int CPL>
__global__ __launch_bounds__(256) void splitk_resid_kernel(const float* __restrict__ parts, int nsplit, size_t slice_stride, const float* __restrict__ bias,
                                                           resid_t* __restrict__ x, float2* __restrict__ stats_out, int M) {
    constexpr int d = CPL * 64, GL = 96 / CPL;                  // lanes per statistics group (8 at d = 768, 16 at d = 384)
    static_assert(96 % CPL == 0 && (GL & (GL - 1)) == 0 && CPL % 2 == 0, "a 96-column group must be a power-of-two run of lanes");
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    float v[CPL];
#pragma unroll
    for (int c = 0; c < CPL; c += 2) {
        const float2 b2 = *reinterpret_cast<const float2*>(bias + CPL * lane + c);
        v[c] = b2.x; v[c + 1] = b2.y;
    }
    for (int sp = 0; sp < nsplit; ++sp) {
        const float* src = parts + sp * slice_stride + (size_t)row * d + CPL * lane;
#pragma unroll
        for (int c = 0; c < CPL; c += 2) {
            const float2 t = *reinterpret_cast<const float2*>(src + c);
            v[c] += t.x; v[c + 1] += t.y;
        }
    }
    resid_t* px = x + (size_t)row * d + CPL * lane;
    float su = 0.f, sq = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; c += 2) {
        const float2 xv = rs_load2(px + c);
        const float o0 = xv.x + v[c], o1 = xv.y + v[c + 1];
        rs_store2(px + c, make_float2(o0, o1));
        const float r0 = rs_round(o0), r1 = rs_round(o1);
        su += r0 + r1;
        sq = fmaf(r0, r0, fmaf(r1, r1, sq));
    }
    if (stats_out) {
#pragma unroll
        for (int o2 = 1; o2 < GL; o2 <<= 1) { su += __shfl_xor(su, o2, 64); sq += __shfl_xor(sq, o2, 64); }
        const int slot = lane / GL;
        if ((lane & (GL - 1)) == 0 && slot < kLnSlots) stats_out[(size_t)row * kLnSlots + slot] = make_float2(su, sq);
    }
}

void launch_splitk_resid(const float* parts, int nsplit, size_t slice_stride, const float* bias, resid_t* x, float2* stats_out, int M, int d, hipStream_t s) {
    const SplitkFinishPlan f = plan_splitk_finish(M, d);
    const dim3 grid(f.gx), block(f.block);
    note_paths(f.paths);
    if (f.form == SKF_CPL12) hipLaunchKernelGGL(splitk_resid_kernel<12>, grid, block, 0, s, parts, nsplit, slice_stride, bias, x, stats_out, M);
    else if (f.form == SKF_CPL6) hipLaunchKernelGGL(splitk_resid_kernel<6>, grid, block, 0, s, parts, nsplit, slice_stride, bias, x, stats_out, M);
}

void launch_tail(const TailParams& p, hipStream_t s) {
    const TailPlan t = plan_tail(p.batch, p.ntok, p.pd, p.d, p.hid != nullptr, p.w_hl != nullptr, device_cu_count());
    const dim3 grid(t.gx), block(t.block);
    note_paths(t.paths);
#ifdef TLD_RESID_BF16
    if (t.form == TAIL_FOLD) {
#define TLD_TF(NT, RT) hipLaunchKernelGGL((tail_fold_kernel<NT, RT>), grid, block, t.lds, s, p)
        switch (t.nt) {
            case 1: if (t.rt == 1) TLD_TF(1, 1); else TLD_TF(1, 4); break;
            case 2: if (t.rt == 1) TLD_TF(2, 1); else TLD_TF(2, 4); break;
            case 3: if (t.rt == 1) TLD_TF(3, 1); else TLD_TF(3, 2); break;
            default: if (t.rt == 1) TLD_TF(4, 1); else TLD_TF(4, 2); break;
        }
#undef TLD_TF
        return;
    }
    if (t.form == TAIL_MFMA) {
#define TLD_TM(NT) do { TLD_LDS_OPT_IN((tail_mfma_kernel<NT>), t.lds); hipLaunchKernelGGL((tail_mfma_kernel<NT>), grid, block, t.lds, s, p, p.w_hl); } while (0)
        switch (t.nt) { case 1: TLD_TM(1); break; case 2: TLD_TM(2); break; case 3: TLD_TM(3); break; default: TLD_TM(4); break; }
#undef TLD_TM
        return;
    }
#endif
    TLD_DISPATCH_D(p.d, { TLD_LDS_OPT_IN((tail_kernel<NJ, HALF>), t.lds); hipLaunchKernelGGL((tail_kernel<NJ, HALF>), grid, block, t.lds, s, p, t.rows_per_block); });
}

#ifdef TLD_RESID_BF16
void launch_tail_fold_debug_row(float* row, const resid_t* x, const float* bias, int M, int d, hipStream_t s) {
    const int64_t n = (int64_t)M * d;
    hipLaunchKernelGGL(tail_fold_debug_row_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, row, x, bias, n, d);
}
#endif

namespace {
bool aligned16(const void* a) { return (reinterpret_cast<uintptr_t>(a) & 15) == 0; }
// a runtime boolean, or an index below 4, as a compile-time constant: f(std::bool_constant<b>{}), f(std::integral_constant<int, i>{})
template <class F> void with_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
template <class F> void with_index4(int i, F&& f) {
    switch (i) {
        case 0: f(std::integral_constant<int, 0>{}); break;
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        default: f(std::integral_constant<int, 3>{}); break;
    }
}
}

void launch_sampler_step(const SamplerStepParams& p, int path, hipStream_t s, bool slots) {
    const int n = p.active * p.img;
    // 16-byte accesses: four consecutive elements then share a sample, a channel and one aligned mask quad (null pointers count as aligned)
    const bool vec = p.img % 4 == 0 && p.chan_stride % 4 == 0 && aligned16(p.x0_2b) && aligned16(p.x_t) && aligned16(p.x0_prev) && aligned16(p.out_latent) &&
                     aligned16(p.trace_x0) && aligned16(p.trace_xt) && aligned16(p.noise) && aligned16(p.z0) && aligned16(p.mask) && aligned16(p.shape_mom);
    const int threads = vec ? n / 4 : n;
    const dim3 grid((threads + 255) / 256), block(256);
    note_path(path);
    if (p.req_slot) {       // the session flavour: SLOT, with or without NOISE; no mask, no shape, no traces (tld_session_step passes none)
        with_bool(vec, [&](auto v4) {
            with_bool(p.noise_rows != nullptr, [&](auto nz) {
                hipLaunchKernelGGL((sampler_step_kernel<false, decltype(v4)::value ? 4 : 1, true, decltype(nz)::value, false, true>), grid, block, 0, s, p);
            });
        });
        return;
    }
    // the flavours nest: plain, SLOT, SLOT + NOISE, SLOT + NOISE + SHAPE
    const int flavour = !slots ? 0 : !p.noise_rows ? 1 : !p.shape_rows ? 2 : 3;
    with_bool(p.mask != nullptr, [&](auto mask) {
        with_bool(vec, [&](auto v4) {
            with_index4(flavour, [&](auto f) {
                constexpr int F = decltype(f)::value;
                hipLaunchKernelGGL((sampler_step_kernel<decltype(mask)::value, decltype(v4)::value ? 4 : 1, (F >= 1), (F >= 2), (F >= 3)>), grid, block, 0, s, p);
            });
        });
    });
}

void launch_guidance_stats(const GuidanceStatsParams& p, hipStream_t s) {
    const bool vec = p.img % 4 == 0 && aligned16(p.cond) && aligned16(p.unc_base) && aligned16(p.mom);
    if (vec) hipLaunchKernelGGL((guidance_stats_kernel<4>), dim3((unsigned)p.active), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((guidance_stats_kernel<1>), dim3((unsigned)p.active), dim3(256), 0, s, p);
}

void launch_guidance_shape_debug(const float* cond, const float* unc, float* mom, const SamplerStepRow* rows, const GuidanceShape* shape_rows,
                                 const float2* pq, int batch, int img, float* x0, hipStream_t s) {
    const int64_t n = (int64_t)batch * img;
    hipLaunchKernelGGL(guidance_shape_debug_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, cond, unc, mom, rows, shape_rows, pq, batch, img, x0);
}

void launch_sampler_noise_debug(const uint64_t* keys, const uint32_t* steps, int batch, int img, float* z, hipStream_t s) {
    const int64_t threads = (int64_t)batch * ((img + 3) / 4);
    hipLaunchKernelGGL(sampler_noise_debug_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, keys, steps, batch, img, z);
}

void launch_start_mix(const float* noise, const float* z0, const float* s0v, int s0_stride, float* x_t, int batch, int img, int path, hipStream_t s) {
    const int n = batch * img;
    note_path(path);
    if (img % 4 == 0 && aligned16(noise) && aligned16(z0) && aligned16(x_t))
        hipLaunchKernelGGL((start_mix_kernel<4>), dim3((n / 4 + 255) / 256), dim3(256), 0, s, noise, z0, s0v, s0_stride, x_t, n, img);
    else
        hipLaunchKernelGGL((start_mix_kernel<1>), dim3((n + 255) / 256), dim3(256), 0, s, noise, z0, s0v, s0_stride, x_t, n, img);
}

// Streaming form of the same computation for grids that are a multiple of 32 wide (512 / 1024 px latents; round 3): one workgroup =
// one sample x 64 channels x a 32-column strip, walking DOWN the image.  The tiled kernel above loads an 18 x 18 halo tile, waits, computes,
// stores -- 1.27 x the input bytes and three phases per workgroup that only other workgroups can overlap (107 us = 3.8 TB/s at C3).  Here
//   * a fifth wave does nothing but DMA: image row r (32 tokens x 128 B = four 1-KiB pieces, + one halo token per inner strip edge) goes
//     into slot r % NR of an LDS ring, 4 - 5 rows ahead of its first use, with a counted vmcnt of its own (the four computing waves'
//     vmcnt sees only their stores, which nobody waits for);
//   * the computing waves keep the 3-row window in REGISTERS (a thread owns 2 adjacent columns x 4 channels): every input row is read from
//     LDS once and from memory once (1.0 x, + 1/32 per inner strip edge), one barrier per row;
//   * image borders: row -1 / row g are zero registers, columns -1 / g zeroed LDS cells the DMA never writes.
// Same halved taps, bias and half-argument GELU as the tiled kernel, same fp8 output option.
template <bool F8OUT>
__global__ __launch_bounds__(320, 4) void dwconv_gelu_stream_kernel(const bf16* __restrict__ in, bf16* __restrict__ out,
                                                                 const float* __restrict__ w9c, const float* __restrict__ bias, int batch,
                                                                 int g, int C, uint8_t* __restrict__ out8, uint8_t* __restrict__ scale8) {
    constexpr int SW = 32, NR = 7, PF = NR - 1;
    constexpr int RPITCH = (SW + 2) * 128;                  // one ring row: tokens j0 - 1 .. j0 + 32
    __shared__ __attribute__((aligned(16))) char ring[NR * RPITCH];
    typedef const __attribute__((address_space(1))) void* gp_t;
    typedef __attribute__((address_space(3))) void* lp_t;
    const int nchunk = C / DW_CB, strips = g / SW;
    int bid = blockIdx.x;
    const int cc = bid % nchunk; bid /= nchunk;
    const int sx = bid % strips;
    const int b = bid / strips;
    const int j0 = sx * SW;
    const bool edge_l = sx > 0, edge_r = sx + 1 < strips;   // inner strip edges: a halo token comes from the neighbouring strip
    const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bf16* src = in + (size_t)b * g * g * C + cc * DW_CB;

    // image columns -1 / g: zero cells (never written by the DMA)
    if (threadIdx.x < NR * 32) {
        const int r = threadIdx.x >> 5, w = threadIdx.x & 31;
        if (!edge_l) *reinterpret_cast<unsigned*>(ring + r * RPITCH + w * 4) = 0u;
        if (!edge_r) *reinterpret_cast<unsigned*>(ring + r * RPITCH + (SW + 1) * 128 + w * 4) = 0u;
    }
    auto stage_row = [&](int r) {       // producer wave only
        char* dst = ring + (r % NR) * RPITCH;
        const bf16* rp = src + ((size_t)r * g + j0) * C + (lane & 7) * 8;
#pragma unroll
        for (int pc = 0; pc < 4; ++pc)
            __builtin_amdgcn_global_load_lds((gp_t)(rp + (size_t)(pc * 8 + (lane >> 3)) * C), (lp_t)(dst + 128 + pc * 1024), 16, 0, 0);
        if (lane < 8) {                 // (both halo loads are issued by every row of a strip with that edge: the count per row is uniform)
            if (edge_l) __builtin_amdgcn_global_load_lds((gp_t)(rp - C), (lp_t)dst, 16, 0, 0);
            if (edge_r) __builtin_amdgcn_global_load_lds((gp_t)(rp + (size_t)SW * C), (lp_t)(dst + (SW + 1) * 128), 16, 0, 0);
        }
    };
    const int ndma = 4 + (edge_l ? 1 : 0) + (edge_r ? 1 : 0);
    // before barrier B_y rows <= y + 5 have been issued and rows <= y + 1 must have landed: at most PF - 2 = 4 rows may still be in flight
    auto wait_rows = [&]() {
        if (ndma == 4) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 * (PF - 2)) : "memory");
        else if (ndma == 5) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(5 * (PF - 2)) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(6 * (PF - 2)) : "memory");
    };
    __syncthreads();                    // zero cells written before any row is read

    if (wid == 4) {
        // ---- producer: rows 0 .. PF up front, then one row per barrier
        for (int r = 0; r <= PF && r < g; ++r) stage_row(r);
        for (int y = 0; y < g; ++y) {
            if (y + PF + 1 >= g) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // tail: fewer rows in flight than the counted wait assumes
            else wait_rows();
            __builtin_amdgcn_s_barrier();                    // B_y: rows <= y + 1 are in LDS; slot of row y is free
            if (y >= 1 && y + PF < g) stage_row(y + PF);
        }
        return;
    }
    // ---- four computing waves: thread = channel quad cq x column pair cg
    const int cq = threadIdx.x & 15, cg = threadIdx.x >> 4;
    const int c0 = cc * DW_CB + cq * 4;
    f32x2 w[9][2], bs[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float4 t = *reinterpret_cast<const float4*>(w9c + (size_t)k * C + c0);
        w[k][0] = f32x2{t.x, t.y}; w[k][1] = f32x2{t.z, t.w};
    }
    {
        const float4 t = *reinterpret_cast<const float4*>(bias + c0);
        bs[0] = f32x2{t.x, t.y}; bs[1] = f32x2{t.z, t.w};
    }
    // window rows: [column 2 cg - 1 .. 2 cg + 2][channel pair]
    f32x2 R0[4][2], R1[4][2], R2[4][2];
    auto zero_row = [&](f32x2 (&R)[4][2]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { R[k][0] = f32x2{0.f, 0.f}; R[k][1] = f32x2{0.f, 0.f}; }
    };
    auto read_row = [&](int r, f32x2 (&R)[4][2]) {
        const char* rp = ring + (r % NR) * RPITCH + (2 * cg) * 128 + cq * 8;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bf16x4 v = *reinterpret_cast<const bf16x4*>(rp + k * 128);
            R[k][0] = f32x2{(float)v[0], (float)v[1]};
            R[k][1] = f32x2{(float)v[2], (float)v[3]};
        }
    };
    // output addresses as running pointers, one add per image row (round 6: `row * C + c0` and the scale index rebuilt per output column were ~20 integer
    // instructions -- 64-bit multiplies among them -- of the ~90 per column of this VALU-bound loop)
    // (32-bit byte offsets from the uniform bases: the engine keeps max_batch x tokens x 4 d x 2 B below 4 GiB, tld_engine_create)
    const size_t orow0 = (size_t)b * g * g + j0 + 2 * cg;
    unsigned ooff = (unsigned)((orow0 * C + c0) * (F8OUT ? 1 : 2));                       // this lane's output column 2 cg of image row y, bytes
    unsigned soff = F8OUT ? (unsigned)mx8_scale_index(c0, orow0, (size_t)batch * g * g) : 0u;
    const unsigned ostride = (unsigned)g * (unsigned)C * (F8OUT ? 1u : 2u);               // bytes per image row
    auto emit = [&](const f32x2 (&U)[4][2], const f32x2 (&M)[4][2], const f32x2 (&D)[4][2]) {
#pragma unroll
        for (int oc = 0; oc < 2; ++oc) {                     // output column 2 cg + oc: window columns oc .. oc + 2
            f32x2 a[2] = {bs[0], bs[1]};
#pragma unroll
            for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    a[h2] = __builtin_elementwise_fma(w[0 + dx][h2], U[oc + dx][h2], a[h2]);
                    a[h2] = __builtin_elementwise_fma(w[3 + dx][h2], M[oc + dx][h2], a[h2]);
                    a[h2] = __builtin_elementwise_fma(w[6 + dx][h2], D[oc + dx][h2], a[h2]);
                }
            a[0] = gelu_erf_fast2_half(a[0]); a[1] = gelu_erf_fast2_half(a[1]);
            bf16x4 o;
            o[0] = (bf16)a[0][0]; o[1] = (bf16)a[0][1]; o[2] = (bf16)a[1][0]; o[3] = (bf16)a[1][1];
            if constexpr (F8OUT) {
                int e8;
                const unsigned pk = mx8_pack4((float)o[0], (float)o[1], (float)o[2], (float)o[3], &e8);
                *reinterpret_cast<unsigned*>(out8 + ooff + (unsigned)(oc * C)) = pk;
                if ((cq & 7) == 0) scale8[soff + oc * 4] = (uint8_t)e8;
            } else {
                *reinterpret_cast<bf16x4*>(reinterpret_cast<char*>(out) + ooff + (unsigned)(oc * C * 2)) = o;
            }
        }
        ooff += ostride;
        if constexpr (F8OUT) soff += (unsigned)g * 4u;
    };
    zero_row(R0);                                            // image row -1
    __builtin_amdgcn_s_barrier();                            // B_0: rows 0, 1 landed
    read_row(0, R1);
    // three named window rows rotate (no register copies): y, y + 1, y + 2 per trip
    auto step = [&](f32x2 (&U)[4][2], f32x2 (&M)[4][2], f32x2 (&D)[4][2], int y) {
        if (y > 0) __builtin_amdgcn_s_barrier();             // B_y
        if (y + 1 < g) read_row(y + 1, D); else zero_row(D);
        emit(U, M, D);
    };
    int y = 0;
    for (; y + 3 <= g; y += 3) {
        step(R0, R1, R2, y);
        step(R1, R2, R0, y + 1);
        step(R2, R0, R1, y + 2);
    }
    if (y < g) { step(R0, R1, R2, y); ++y; }
    if (y < g) { step(R1, R2, R0, y); }
}

// ---- seam rows of the depthwise conv fused into the up-projection at 32 x 32 tokens (GemmParams::dw_grid = 32, tld_gemm.hip) ----------------------
// A 256-row GEMM tile is 8 rows of the image; its epilogue finishes rows 1 .. 6 (and the image's own border rows) and leaves its hidden rows 0, 1, 6, 7
// in `seam` as token-pair dwords: [tile][column tile][64 pair-rows: rows 0, 1, 6, 7 x 16 pair-columns][256 channels].  Here: the output rows on either
// side of each of a sample's three tile seams -- window rows (6, 7) of the upper tile and (0, 1) of the lower one -- with the epilogue's own tap
// arithmetic (halved taps as packed bf16 pairs, v_dot2 accumulation in fp32, GELU of twice the argument).  One workgroup per (sample, seam, column
// tile): 64 channel quads x 4 column quarters.
__global__ __launch_bounds__(256) void dwconv_seam_kernel(const uint32_t* __restrict__ seam, const uint32_t* __restrict__ wpk, const float* __restrict__ bias_half,
                                                          bf16* __restrict__ out, int ldo, int channels) {
    const int ntn = channels >> 8;
    int bid = blockIdx.x;
    const int n = bid % ntn; bid /= ntn;
    const int sm = bid % 3, b = bid / 3;
    const int cq = threadIdx.x & 63, qq = threadIdx.x >> 6;
    const int c0 = n * 256 + cq * 4;
    const uint32_t* lo = seam + ((size_t)(b * 4 + sm) * ntn + n) * (64 * 256) + cq * 4;        // upper tile: its rows 6, 7 are pair-rows 32 .. 63
    const uint32_t* hi = seam + ((size_t)(b * 4 + sm + 1) * ntn + n) * (64 * 256) + cq * 4;    // lower tile: its rows 0, 1 are pair-rows 0 .. 31
    u32x4 WA[3], WB[3], WC[3], WD[3];
#pragma unroll
    for (int du = 0; du < 3; ++du) {
        WA[du] = *reinterpret_cast<const u32x4*>(wpk + (size_t)(du * 4 + 0) * channels + c0);
        WB[du] = *reinterpret_cast<const u32x4*>(wpk + (size_t)(du * 4 + 1) * channels + c0);
        WC[du] = *reinterpret_cast<const u32x4*>(wpk + (size_t)(du * 4 + 2) * channels + c0);
        WD[du] = *reinterpret_cast<const u32x4*>(wpk + (size_t)(du * 4 + 3) * channels + c0);
    }
    const float4 bsv = *reinterpret_cast<const float4*>(bias_half + c0);
    const f32x4 bs = {bsv.x, bsv.y, bsv.z, bsv.w};
    // the six pair-columns 4 qq - 1 .. 4 qq + 4 of the four window rows (zero outside the image)
    u32x4 w[6][4];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int q = 4 * qq - 1 + k;
        const bool ok = q >= 0 && q < 16;
        const int qc = ok ? q : 0;
        const u32x4 z = {0u, 0u, 0u, 0u};
        w[k][0] = ok ? *reinterpret_cast<const u32x4*>(lo + (size_t)(32 + qc) * 256) : z;
        w[k][1] = ok ? *reinterpret_cast<const u32x4*>(lo + (size_t)(48 + qc) * 256) : z;
        w[k][2] = ok ? *reinterpret_cast<const u32x4*>(hi + (size_t)qc * 256) : z;
        w[k][3] = ok ? *reinterpret_cast<const u32x4*>(hi + (size_t)(16 + qc) * 256) : z;
    }
    auto dot2 = [](unsigned a, unsigned b2, float c) {
        return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b2), c, false);
    };
    bf16* dst0 = out + ((size_t)b * 1024 + (size_t)(8 * sm + 7) * 32) * ldo + c0;             // image row 8 sm + 7; the next row is 32 tokens on
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u32x4 (&L)[4] = w[k]; const u32x4 (&Mc)[4] = w[k + 1]; const u32x4 (&R)[4] = w[k + 2];
        const int q = 4 * qq + k;
#pragma unroll
        for (int rr = 0; rr < 2; ++rr) {
            f32x4 ae = bs, ao = bs;
#pragma unroll
            for (int du = 0; du < 3; ++du)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    ae[ch] = dot2(L[rr + du][ch], WA[du][ch], ae[ch]);
                    ao[ch] = dot2(Mc[rr + du][ch], WC[du][ch], ao[ch]);
                    ae[ch] = dot2(Mc[rr + du][ch], WB[du][ch], ae[ch]);
                    ao[ch] = dot2(R[rr + du][ch], WD[du][ch], ao[ch]);
                }
            f32x2 e0 = {ae[0], ae[1]}, e1 = {ae[2], ae[3]}, o0 = {ao[0], ao[1]}, o1 = {ao[2], ao[3]};
            e0 = gelu_erf_fast2_half(e0); e1 = gelu_erf_fast2_half(e1);
            o0 = gelu_erf_fast2_half(o0); o1 = gelu_erf_fast2_half(o1);
            bf16x4 oe, oo;
            oe[0] = (bf16)e0[0]; oe[1] = (bf16)e0[1]; oe[2] = (bf16)e1[0]; oe[3] = (bf16)e1[1];
            oo[0] = (bf16)o0[0]; oo[1] = (bf16)o0[1]; oo[2] = (bf16)o1[0]; oo[3] = (bf16)o1[1];
            *reinterpret_cast<bf16x4*>(dst0 + ((size_t)rr * 32 + 2 * q) * ldo) = oe;
            *reinterpret_cast<bf16x4*>(dst0 + ((size_t)rr * 32 + 2 * q + 1) * ldo) = oo;
        }
    }
}

void launch_dwconv_seam(const uint32_t* seam, const uint32_t* dw_wpk, const float* dw_b_half, bf16* out, int ldo, int batch, int channels, hipStream_t s) {
    hipLaunchKernelGGL(dwconv_seam_kernel, dim3((unsigned)(batch * 3 * (channels >> 8))), dim3(256), 0, s, seam, dw_wpk, dw_b_half, out, ldo, channels);
}

void launch_dwconv_gelu(const bf16* in, bf16* out, const float* w9c, const float* bias, const float* w9c_half,
                        const float* bias_half, int batch, int grid, int channels, hipStream_t s, uint8_t* out8,
                        uint8_t* scale8) {
    const DwconvPlan w = plan_dwconv(batch, grid, channels, out8 != nullptr);
    const dim3 gr(w.gx), block(w.block);
    note_paths(w.paths);
    switch (w.form) {       // the streaming and the tiled kernel take the halved tables
        case DW_STREAM:
            if (w.f8) hipLaunchKernelGGL(dwconv_gelu_stream_kernel<true>, gr, block, 0, s, in, out, w9c_half, bias_half, batch, grid, channels, out8, scale8);
            else hipLaunchKernelGGL(dwconv_gelu_stream_kernel<false>, gr, block, 0, s, in, out, w9c_half, bias_half, batch, grid, channels, out8, scale8);
            break;
        case DW_TILED:
            if (w.f8) hipLaunchKernelGGL(dwconv_gelu_tiled_kernel<true>, gr, block, 0, s, in, out, w9c_half, bias_half, batch, grid, channels, out8, scale8);
            else hipLaunchKernelGGL(dwconv_gelu_tiled_kernel<false>, gr, block, 0, s, in, out, w9c_half, bias_half, batch, grid, channels, out8, scale8);
            break;
        case DW_WHOLE: hipLaunchKernelGGL(dwconv_gelu_kernel, gr, block, w.lds, s, in, out, w9c, bias, batch, grid, channels); break;
    }
}

}  // namespace tld

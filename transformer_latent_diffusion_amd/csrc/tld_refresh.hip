// tld_refresh.hip -- every weight image of the inference engine, built on the device from a flat fp32 parameter vector: THE one builder, run by
// tld_engine_finalize_weights on the loaded state dict and by tld_engine_refresh_weights on a caller's vector.
//
// The kernels write into the buffers finalize allocated (a null pointer: an image this engine's mode does not hold).  Every image is DEFINED to the bit,
// and tests/weight_image_refs.py restates each definition in numpy; tests/test_gpu_weight_refresh.py compares the engine's images with it using ==.
// What the definitions fix:
//   * one bf16 and one e4m3 rounding, in integer arithmetic (tld_refresh_math.h; the host's f32_to_bf16_rne and quant_mx8_host round alike), no hardware
//     convert;
//   * the two double-precision sums of a LayerNorm fold are sequential per output row, k = 0 .. d - 1, one add per element: one lane walks one row
//     (refresh_fold_kernel).  A tree would change the last bit of float(sum) once in some tens of millions of elements;
//   * contraction is off in every kernel here (a product of two fp32 values is exact in double, so it could not change the sums; pinned anyway).
// No kernel reads the vector past its last parameter: 16-byte loads are taken only where the element count and both addresses allow them.
// Up to five launches per refresh: the images outside the blocks, the blocks' elementwise images, the folds, the folded out_proj operand, the e4m3 images; the blocks sit a constant
// stride apart in the flat vector, so the last three take the block index from blockIdx.z.  All stores are ordinary vector stores.
#include "tld_common.h"
#include "tld_stages.h"      // fail
#include "tld_refresh.h"
#include "tld_refresh_math.h"
#include "tld_tail_fold_math.h"

namespace tld {

namespace {

struct RefreshJobs { RefreshJob job[kRefreshMaxJobs]; };

__device__ __forceinline__ uint16_t bf16_bits(float f) { return bf16_rne_bits(__float_as_uint(f)); }
__device__ __forceinline__ float bf16_value(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }

// dst[i] = src[i], i in [0, n), by the whole grid row (tid of nth threads); 16-byte accesses where both ends allow them
__device__ __forceinline__ void copy_f32(float* __restrict__ dst, const float* __restrict__ src, int64_t n, int64_t tid, int64_t nth) {
    if (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0 && (n & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int64_t i = tid; i < (n >> 2); i += nth) d4[i] = s4[i];
    } else {
        for (int64_t i = tid; i < n; i += nth) dst[i] = src[i];
    }
}

// dst[i] = bf16(src[i])
__device__ __forceinline__ void cast_bf16(uint16_t* __restrict__ dst, const float* __restrict__ src, int64_t n, int64_t tid, int64_t nth) {
    if (((reinterpret_cast<uintptr_t>(src) & 15) | (reinterpret_cast<uintptr_t>(dst) & 7)) == 0 && (n & 3) == 0) {
        const float4* s4 = reinterpret_cast<const float4*>(src);
        uint2* d2 = reinterpret_cast<uint2*>(dst);
        for (int64_t i = tid; i < (n >> 2); i += nth) {
            const float4 v = s4[i];
            d2[i] = make_uint2((uint32_t)bf16_bits(v.x) | ((uint32_t)bf16_bits(v.y) << 16), (uint32_t)bf16_bits(v.z) | ((uint32_t)bf16_bits(v.w) << 16));
        }
    } else {
        for (int64_t i = tid; i < n; i += nth) dst[i] = bf16_bits(src[i]);
    }
}

// ---- the images outside the blocks: blockIdx.y = job ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void refresh_globals_kernel(RefreshJobs J, const float* __restrict__ flat) {
#pragma clang fp contract(off)
    const RefreshJob& j = J.job[blockIdx.y];
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
    const float* src = flat + j.src;
    if (j.kind == RJ_COPY) {
        copy_f32(static_cast<float*>(j.dst), src, j.n, tid, nth);
    } else if (j.kind == RJ_SPLIT_HL) {
        uint16_t* dst = static_cast<uint16_t*>(j.dst);
        for (int64_t i = tid; i < j.n; i += nth) {
            const float w = src[i];
            const uint16_t hi = bf16_bits(w);
            dst[i] = hi;
            dst[j.n + i] = bf16_bits(w - bf16_value(hi));
        }
    } else {      // RJ_TRANSPOSE: [rows][cols] -> [cols][rows] (d x patch_dim: small)
        float* dst = static_cast<float*>(j.dst);
        const int64_t cols = j.cols, rows = j.n / cols;
        for (int64_t i = tid; i < j.n; i += nth) {
            const int64_t r = i / cols, c = i - r * cols;
            dst[c * rows + r] = src[i];
        }
    }
}

// ---- a block's elementwise images: blockIdx.y = image, blockIdx.z = block ------------------------------------------------------------------
enum { LJ_KV = 0, LJ_Q, LJ_UP_B, LJ_DW_B, LJ_DOWN_B, LJ_N1W, LJ_N1B, LJ_N2W, LJ_N2B, LJ_N3W, LJ_N3B, LJ_QKV_BF16, LJ_UP_BF16, LJ_DOWN_BF16, LJ_DW, LJ_COUNT };

__global__ __launch_bounds__(256) void refresh_layer_kernel(const Layer* __restrict__ layers, const float* __restrict__ flat, LayerOffsets o, int64_t stride,
                                                            int d, int hid) {
#pragma clang fp contract(off)
    const Layer& Ly = layers[blockIdx.z];
    const float* base = flat + (int64_t)blockIdx.z * stride;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
    const int64_t dd = (int64_t)d * d, hd = (int64_t)hid * d;
    switch (blockIdx.y) {
    case LJ_KV: copy_f32(Ly.kv_w, base + o.kv, 2 * dd, tid, nth); break;
    case LJ_Q: copy_f32(Ly.q_w, base + o.q, dd, tid, nth); break;
    case LJ_UP_B: copy_f32(Ly.up_b, base + o.up_b, hid, tid, nth); break;
    case LJ_DW_B: copy_f32(Ly.dw_b, base + o.dw_b, hid, tid, nth); break;
    case LJ_DOWN_B: copy_f32(Ly.down_b, base + o.down_b, d, tid, nth); break;
    case LJ_N1W: copy_f32(Ly.n1_w, base + o.n1w, d, tid, nth); break;
    case LJ_N1B: copy_f32(Ly.n1_b, base + o.n1b, d, tid, nth); break;
    case LJ_N2W: copy_f32(Ly.n2_w, base + o.n2w, d, tid, nth); break;
    case LJ_N2B: copy_f32(Ly.n2_b, base + o.n2b, d, tid, nth); break;
    case LJ_N3W: copy_f32(Ly.n3_w, base + o.n3w, d, tid, nth); break;
    case LJ_N3B: copy_f32(Ly.n3_b, base + o.n3b, d, tid, nth); break;
    case LJ_QKV_BF16: if (Ly.qkv_w) cast_bf16(reinterpret_cast<uint16_t*>(Ly.qkv_w), base + o.qkv, 3 * dd, tid, nth); break;
    case LJ_UP_BF16: if (Ly.up_w) cast_bf16(reinterpret_cast<uint16_t*>(Ly.up_w), base + o.up_w, hd, tid, nth); break;
    case LJ_DOWN_BF16: if (Ly.down_w) cast_bf16(reinterpret_cast<uint16_t*>(Ly.down_w), base + o.down_w, hd, tid, nth); break;
    default: {    // LJ_DW: depthwise taps [hid][9] -> [9][hid], their halves, the halved bias, and the halved taps as packed bf16 pairs [3][4][hid]:
        // per window row du with halved taps (w0, w1, w2): kind 0 = (lo 0, hi w0), 1 = (w1, w2), 2 = (w0, w1), 3 = (w2, 0)
        const float* w = base + o.dw_w;
        const float* b = base + o.dw_b;
        for (int64_t c = tid; c < hid; c += nth) {
            uint32_t h[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float t = w[c * 9 + k], th = t * 0.5f;
                Ly.dw_w9c[(int64_t)k * hid + c] = t;
                Ly.dw_w9c_half[(int64_t)k * hid + c] = th;
                h[k] = bf16_bits(th);
            }
            Ly.dw_b_half[c] = b[c] * 0.5f;
#pragma unroll
            for (int du = 0; du < 3; ++du) {
                const uint32_t w0 = h[du * 3], w1 = h[du * 3 + 1], w2 = h[du * 3 + 2];
                Ly.dw_wpk[(int64_t)(du * 4 + 0) * hid + c] = w0 << 16;
                Ly.dw_wpk[(int64_t)(du * 4 + 1) * hid + c] = w1 | (w2 << 16);
                Ly.dw_wpk[(int64_t)(du * 4 + 2) * hid + c] = w0 | (w1 << 16);
                Ly.dw_wpk[(int64_t)(du * 4 + 3) * hid + c] = w2;
            }
        }
    } }
}

// ---- the LayerNorm folds: blockIdx.y = 0 LayerNorm-1 into Wqkv [3d][d], 1 LayerNorm-3 into Wup [hid][d]; blockIdx.z = block ------------------
//   wf[n][k] = bf16(g[k] * W[n][k])          (the product rounded to fp32 first)
//   c1[n]    = (float) sum_k double(float(wf[n][k]))
//   b1[n]    = (float) (sum_k double(be[k]) * double(W[n][k])  [+ double(up_b[n]) for LayerNorm-3])
// One wave owns 64 rows.  Per 64-column tile: lane j loads column j of the 64 rows (256-byte coalesced runs), stores wf (and its packed copy) and parks
// W in LDS; then lane r walks row r of the tile in k order, re-deriving wf from g (an LDS broadcast) -- so both sums are the sequential sums of the definition.
// The pitch of 65 floats keeps the walk (lane r at word 65 r + k) off bank conflicts.
__global__ __launch_bounds__(64) void refresh_fold_kernel(const Layer* __restrict__ layers, const float* __restrict__ flat, LayerOffsets o, int64_t stride, int d,
                                                          int hid) {
#pragma clang fp contract(off)
    __shared__ float tile[64][65];
    __shared__ float gs[64], bs[64];
    const Layer& Ly = layers[blockIdx.z];
    const bool ln3 = blockIdx.y == 1;
    uint16_t* wf = reinterpret_cast<uint16_t*>(ln3 ? Ly.up_wf : Ly.qkv_wf);
    const int R = ln3 ? hid : 3 * d, row0 = blockIdx.x * 64;
    if (!wf || row0 >= R) return;              // (uniform over the workgroup: before any barrier)
    const float* base = flat + (int64_t)blockIdx.z * stride;
    const float* W = base + (ln3 ? o.up_w : o.qkv);
    const float* g = base + (ln3 ? o.n3w : o.n1w);
    const float* be = base + (ln3 ? o.n3b : o.n1b);
    const int lane = threadIdx.x;
    // rows [q; k; v] x [head][64] -> [head][feature half][q | k | v][32] (the fused QKV -> attention kernel's order): the 64 rows of this workgroup are
    // one (part, head), since d is a multiple of 64
    uint16_t* wp = ln3 ? nullptr : reinterpret_cast<uint16_t*>(Ly.qkv_wp);
    const int part = row0 / d, head = (row0 - part * d) >> 6;
    auto packed_row = [&](int r) { return head * 192 + (r >> 5) * 96 + part * 32 + (r & 31); };
    uint16_t* wp2 = ln3 ? nullptr : reinterpret_cast<uint16_t*>(Ly.qkv_wp2);      // ... and the two-head form's, where the engine holds it
    double sc = 0.0, sb = 0.0;
    for (int k0 = 0; k0 < d; k0 += 64) {
        const float gk = g[k0 + lane];
        gs[lane] = gk; bs[lane] = be[k0 + lane];
        for (int r0 = 0; r0 < 64; r0 += 16) {      // 16 loads in flight (the stores below could alias them for all the compiler knows)
            float w[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) w[i] = W[(int64_t)(row0 + r0 + i) * d + k0 + lane];
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int r = r0 + i;
                tile[r][lane] = w[i];
                const uint16_t q = bf16_bits(gk * w[i]);
                wf[(int64_t)(row0 + r) * d + k0 + lane] = q;
                if (wp) wp[(int64_t)packed_row(r) * d + k0 + lane] = q;
                if (wp2) wp2[(int64_t)qkv_pair_row(part, head, r) * d + k0 + lane] = q;
            }
        }
        __syncthreads();
        for (int k = 0; k < 64; ++k) {
            const float w = tile[lane][k];
            const float qf = bf16_value(bf16_bits(gs[k] * w));
            sc += (double)qf;
            sb += (double)bs[k] * (double)w;
        }
        __syncthreads();
    }
    const int n = row0 + lane;
    const float c1 = (float)sc;
    const float b1 = ln3 ? (float)(sb + (double)base[o.up_b + n]) : (float)sb;
    (ln3 ? Ly.up_c1 : Ly.qkv_c1)[n] = c1;
    (ln3 ? Ly.up_b1 : Ly.qkv_b1)[n] = b1;
    if (wp) { Ly.qkv_c1p[packed_row(lane)] = c1; Ly.qkv_b1p[packed_row(lane)] = b1; }      // (the 64 pad entries behind them are not touched)
    if (wp2) { Ly.qkv_c1p2[qkv_pair_row(part, head, lane)] = c1; Ly.qkv_b1p2[qkv_pair_row(part, head, lane)] = b1; }
}

// ---- out_proj folded into the last block's down projection: the split bf16 image of [Wout | Wout Wd] and b' = Wout bd + bo -----------------------
// One thread per element, each walking its own sum k-ascending (tld_tail_fold_math.h spells the arithmetic).  Consecutive threads take
// consecutive columns j, so the reads of Wd[k][j] are coalesced and Wout[f][k] is a broadcast.  Items: pd hid folded weights | pd d copies of Wout | pd biases.
__global__ __launch_bounds__(256) void refresh_tail_fold_kernel(bf16* __restrict__ img_, float* __restrict__ bias, const float* __restrict__ wout,
                                                                const float* __restrict__ bo, const float* __restrict__ wd, const float* __restrict__ bd,
                                                                int pd, int d, int hid) {
#pragma clang fp contract(off)
    uint16_t* img = reinterpret_cast<uint16_t*>(img_);
    const int K = d + hid;
    const int64_t lo = (int64_t)tail_fold_padded_rows(pd) * K;
    const int64_t nf = (int64_t)pd * hid, nw = (int64_t)pd * d;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nf + nw) {
        int f, k;
        float w;
        if (i < nf) { f = (int)(i / hid); const int j = (int)(i - (int64_t)f * hid); k = d + j; w = tail_fold_weight(wout + (int64_t)f * d, wd, d, hid, j); }
        else { const int64_t r = i - nf; f = (int)(r / d); k = (int)(r - (int64_t)f * d); w = wout[r]; }
        uint16_t h, l;
        tail_fold_split(w, &h, &l);
        img[(int64_t)f * K + k] = h;
        img[lo + (int64_t)f * K + k] = l;
    } else if (i < nf + nw + pd) {
        const int f = (int)(i - nf - nw);
        bias[f] = tail_fold_bias(wout + (int64_t)f * d, bd, bo[f], d);
    }
}

// ---- MX-fp8 from fp32 (quant_mx8_host, tld_quant.hip): per row and block of 32 K-elements X = 2^(floor(log2 amax) - 8), q = e4m3_rne(clamp(v / X)) ----
// a thread owns 8 consecutive elements, four adjacent lanes one block (K % 32 == 0: a quad never straddles two rows, and the group count is a multiple of 4,
// so a quad is whole or absent)
__device__ __forceinline__ void quant_mx8_f32_rows(const float* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ scale, int rows, int K,
                                                   int64_t tid, int64_t nth) {
    const int gpr = K >> 3;
    const int64_t groups = (int64_t)rows * gpr;
    const bool vec = (reinterpret_cast<uintptr_t>(in) & 15) == 0;
    for (int64_t g = tid; g < groups; g += nth) {
        const int row = (int)(g / gpr), k0 = (int)(g - (int64_t)row * gpr) * 8;
        const float* p = in + (int64_t)row * K + k0;
        float f[8];
        if (vec) {
            const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = p[e];
        }
        float amax = 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf(f[e]));
        amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0xB1, 0xf, 0xf, true)));   // lane ^ 1
        amax = fmaxf(amax, __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(amax), 0x4E, 0xf, 0xf, true)));   // lane ^ 2
        const int e_amax = (int)((__float_as_uint(amax) >> 23) & 0xffu);
        const int e8 = e_amax > 8 ? e_amax - 8 : 0;
        const float inv = __uint_as_float((unsigned)(254 - e8) << 23);            // 1 / X, exact
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float v = f[e] * inv;
            v = v < -448.f ? -448.f : (v > 448.f ? 448.f : v);                    // (a NaN passes, as in quant_mx8_host)
            w[e >> 2] |= (uint32_t)e4m3_rne_bits(__float_as_uint(v)) << ((e & 3) * 8);
        }
        *reinterpret_cast<uint2*>(out + (int64_t)row * K + k0) = make_uint2(w[0], w[1]);
        if ((k0 & 31) == 0) scale[((int64_t)(k0 >> 7) * rows + row) * 4 + ((k0 >> 5) & 3)] = (uint8_t)e8;
    }
}

__global__ __launch_bounds__(256) void quant_mx8_f32_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, uint8_t* __restrict__ scale, int rows, int K) {
#pragma clang fp contract(off)
    quant_mx8_f32_rows(in, out, scale, rows, K, (int64_t)blockIdx.x * 256 + threadIdx.x, (int64_t)gridDim.x * 256);
}

// blockIdx.y = 0 Wqkv [3d][d], 1 Wup [hid][d], 2 Wdown [d][hid]; blockIdx.z = block
__global__ __launch_bounds__(256) void refresh_fp8_kernel(const Layer* __restrict__ layers, const float* __restrict__ flat, LayerOffsets o, int64_t stride, int d,
                                                          int hid) {
#pragma clang fp contract(off)
    const Layer& Ly = layers[blockIdx.z];
    const float* base = flat + (int64_t)blockIdx.z * stride;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
    if (blockIdx.y == 0) { if (Ly.qkv_w8) quant_mx8_f32_rows(base + o.qkv, Ly.qkv_w8, Ly.qkv_s8, 3 * d, d, tid, nth); }
    else if (blockIdx.y == 1) { if (Ly.up_w8) quant_mx8_f32_rows(base + o.up_w, Ly.up_w8, Ly.up_s8, hid, d, tid, nth); }
    else if (Ly.down_w8) quant_mx8_f32_rows(base + o.down_w, Ly.down_w8, Ly.down_s8, d, hid, tid, nth);
}

}  // namespace

int launch_refresh_weights(const RefreshPlan& p, const float* flat, hipStream_t s) {
    RefreshJobs J{};
    for (int i = 0; i < p.njobs; ++i) J.job[i] = p.jobs[i];
    hipLaunchKernelGGL(refresh_globals_kernel, dim3(64, (unsigned)p.njobs), dim3(256), 0, s, J, flat);
    hipLaunchKernelGGL(refresh_layer_kernel, dim3(32, LJ_COUNT, (unsigned)p.L), dim3(256), 0, s, p.layers_dev, flat, p.l0, p.layer_stride, p.d, p.hid);
    if (p.fold) {
        const int rows = p.hid > 3 * p.d ? p.hid : 3 * p.d;
        hipLaunchKernelGGL(refresh_fold_kernel, dim3((unsigned)(rows / 64), 2, (unsigned)p.L), dim3(64), 0, s, p.layers_dev, flat, p.l0, p.layer_stride, p.d, p.hid);
    }
    if (p.tail_fold_hl) {
        const float* last = flat + (int64_t)(p.L - 1) * p.layer_stride;
        const int64_t items = (int64_t)p.pd * (p.hid + p.d + 1);
        hipLaunchKernelGGL(refresh_tail_fold_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, s, p.tail_fold_hl, p.tail_fold_b, flat + p.outw, flat + p.outb,
                           last + p.l0.down_w, last + p.l0.down_b, p.pd, p.d, p.hid);
    }
    if (p.fp8) hipLaunchKernelGGL(refresh_fp8_kernel, dim3(64, 3, (unsigned)p.L), dim3(256), 0, s, p.layers_dev, flat, p.l0, p.layer_stride, p.d, p.hid);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TLD_ERR_HIP, "weight refresh launch failed: %s", hipGetErrorString(e));
    return TLD_OK;
}

void launch_quant_mx8_f32(const float* in, uint8_t* out, uint8_t* scale, int rows, int K, hipStream_t s) {
    const int64_t groups = (int64_t)rows * (K >> 3);
    const unsigned blocks = (unsigned)((groups + 255) / 256 < 4096 ? (groups + 255) / 256 : 4096);
    hipLaunchKernelGGL(quant_mx8_f32_kernel, dim3(blocks), dim3(256), 0, s, in, out, scale, rows, K);
}

}  // namespace tld

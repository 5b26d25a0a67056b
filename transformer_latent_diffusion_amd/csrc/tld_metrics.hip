// tld_metrics.hip -- distribution metrics on embedding banks: tld_feat_append (rows into a zero-padded fp32 bank, L2-normalised
// in double), tld_feat_moments (mean and sample covariance in double, fixed order) and tld_feat_kernel_sum, the all-pairs sum
//     sum_{i < na, j < nb} expm1(-gamma d2_ij),    d2_ij = max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j)
// on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain).  No atomics on any value (the one atomic counts bad rows), no
// partial buffer whose order depends on scheduling: every result repeats bitwise.
//
// Pair kernel geometry: one workgroup of four waves per 128 x 128 tile of the plan (tld_feat_plan.h), each wave 2 x 2 MFMA tiles of 32 x 32, K through
// LDS in chunks of 32 columns ([k][row] images, so the operand reads of a wave are consecutive words).  The row norms come from an fp32 fmaf chain over
// the same LDS images in the same ascending k order -- thread t < 128 owns row t of the a block, thread t >= 128 row t - 128 of the b block -- so that
// a_i . a_i of the MFMA chain and |a_i|^2 are the same bits.  The epilogue forms k - 1 = expm1f(-gamma d2) per pair, removes rows past the end and the
// i == j terms of a same-set diagonal tile by a select on the value, converts to double and only then adds: first the lane's 64 values, then across
// the wave, then the four waves, all in a fixed order.  Ragged ends: row indices are clamped to n - 1 before an address is formed; nothing outside
// rows < n of either operand is read, and the columns read are [0, pitch), which the bank owns.
#include "tld_common.h"
#include "tld_host.h"        // fail, DeviceGuard, HIP_TRY
#include "tld_feat_plan.h"
#include "../../include/tld_hip.h"

#include <algorithm>
#include <cmath>

namespace tld {

namespace {

constexpr int kFeatLdsPitch = FEAT_TILE + 4;       // floats per k row of an LDS image
constexpr int kMomTile = 64;                       // side of a covariance tile
constexpr int kMomRows = 16;                       // rows per LDS stage of the covariance kernel
constexpr int kMeanPhases = 16;                    // row phases of the mean kernel

__device__ __forceinline__ float feat_load(const void* src, int64_t i, int dtype) {
    if (dtype == TLD_DTYPE_F32) return static_cast<const float*>(src)[i];
    const uint16_t h = static_cast<const uint16_t*>(src)[i];
    if (dtype == TLD_DTYPE_BF16) return __builtin_bit_cast(float, (uint32_t)h << 16);
    return (float)__builtin_bit_cast(_Float16, h);
}

// One wave per row.  The squares are exact in double; their sum is taken in ascending column order (lane i of a 64-column group is added i-th, in every
// lane alike), the quotient is formed in double and rounded to fp32 once.
__global__ __launch_bounds__(256) void feat_append_kernel(float* __restrict__ bank, int64_t used, int dim, int pitch, const void* __restrict__ src, int dtype,
                                                          int64_t rows, int normalize, int32_t* __restrict__ bad_count) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t in0 = row * dim;
    double s = 0.0;
    for (int c0 = 0; c0 < dim; c0 += 64) {
        const int c = c0 + lane;
        const float x = feat_load(src, in0 + min(c, dim - 1), dtype);
        const double q = c < dim ? (double)x * (double)x : 0.0;
        const int cnt = min(64, dim - c0);
        for (int i = 0; i < cnt; ++i) s += __shfl(q, i);
    }
    const bool bad = !isfinite(s) || (normalize && s == 0.0);
    const double rn = __dsqrt_rn(s);
    float* out = bank + (used + row) * (int64_t)pitch;
    for (int c = lane; c < pitch; c += 64) {
        const float x = feat_load(src, in0 + min(c, dim - 1), dtype);
        float v = normalize ? (float)__ddiv_rn((double)x, rn) : x;
        v = (bad || c >= dim) ? 0.0f : v;
        out[c] = v;
    }
    if (bad && lane == 0) atomicAdd(bad_count, 1);
}

// mean[c] = (sum over rows) / n.  A workgroup owns 64 columns; wave p adds rows p, p + 16, ... in ascending order and the 16 phase sums are added in
// phase order.
__global__ __launch_bounds__(64 * kMeanPhases) void feat_mean_kernel(const float* __restrict__ bank, int64_t n, int dim, int pitch, double* __restrict__ mean) {
    __shared__ double part[kMeanPhases][64];
    const int lane = threadIdx.x & 63, phase = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane, cc = min(c, dim - 1);
    double s = 0.0;
    for (int64_t r = phase; r < n; r += kMeanPhases) s += (double)bank[r * pitch + cc];
    part[phase][lane] = s;
    __syncthreads();
    if (phase == 0 && c < dim) {
        double t = part[0][lane];
        for (int p = 1; p < kMeanPhases; ++p) t += part[p][lane];
        mean[c] = t / (double)n;
    }
}

// cov[i][j] = sum_r (x_ri - mean_i)(x_rj - mean_j) / (n - 1).  One workgroup owns one 64 x 64 tile and walks all n rows in ascending order; a thread
// owns 4 x 4 entries.  Tile (I, J) and tile (J, I) do the same products in the same order, so cov is symmetric bit for bit.
__global__ __launch_bounds__(256) void feat_cov_kernel(const float* __restrict__ bank, int64_t n, int dim, int pitch, const double* __restrict__ mean,
                                                       double* __restrict__ cov) {
    __shared__ double xi[kMomRows][kMomTile];
    __shared__ double xj[kMomRows][kMomTile];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int i0 = blockIdx.y * kMomTile, j0 = blockIdx.x * kMomTile;
    const int lc = tid & 63, lr = tid >> 6;                    // loader: column lc of rows lr, lr + 4, lr + 8, lr + 12 of the stage
    const int ci = min(i0 + lc, dim - 1), cj = min(j0 + lc, dim - 1);
    const double mi = mean[ci], mj = mean[cj];
    double acc[4][4];
    for (int u = 0; u < 4; ++u) for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int64_t r0 = 0; r0 < n; r0 += kMomRows) {
        __syncthreads();
        for (int q = 0; q < kMomRows / 4; ++q) {
            const int64_t r = r0 + lr + 4 * q;
            const float* p = bank + std::min(r, n - 1) * pitch;
            const double a = (double)p[ci] - mi, b = (double)p[cj] - mj;
            xi[lr + 4 * q][lc] = r < n ? a : 0.0;
            xj[lr + 4 * q][lc] = r < n ? b : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < kMomRows; ++r) {
            double a[4], b[4];
            for (int u = 0; u < 4; ++u) { a[u] = xi[r][ty * 4 + u]; b[u] = xj[r][tx * 4 + u]; }
            for (int u = 0; u < 4; ++u) for (int v = 0; v < 4; ++v) acc[u][v] = fma(a[u], b[v], acc[u][v]);
        }
    }
    const double denom = (double)(n - 1);
    for (int u = 0; u < 4; ++u) for (int v = 0; v < 4; ++v) {
        const int i = i0 + ty * 4 + u, j = j0 + tx * 4 + v;
        if (i < dim && j < dim) cov[(int64_t)i * dim + j] = acc[u][v] / denom;
    }
}

__global__ __launch_bounds__(256) void feat_pair_kernel(const float* __restrict__ a, int64_t na, const float* __restrict__ b, int64_t nb, int pitch, double gamma,
                                                        int same, double* __restrict__ partials) {
    __shared__ float As[FEAT_KCHUNK][kFeatLdsPitch];
    __shared__ float Bs[FEAT_KCHUNK][kFeatLdsPitch];
    __shared__ float nrm[2 * FEAT_TILE];
    __shared__ double wsum[4];
    const FeatTile T = feat_tile_at((int64_t)blockIdx.x, na, nb, same);
    const int64_t r0 = (int64_t)T.ti * FEAT_TILE, c0 = (int64_t)T.tj * FEAT_TILE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
    const int lr = tid >> 3, lc = (tid & 7) * 4;              // loader: 4 columns from lc of rows lr + 32 p
    const float* ap[4];
    const float* bp[4];
    for (int p = 0; p < 4; ++p) {
        ap[p] = a + std::min(r0 + lr + 32 * p, na - 1) * pitch + lc;
        bp[p] = b + std::min(c0 + lr + 32 * p, nb - 1) * pitch + lc;
    }
    f32x4 va[4], vb[4];
    for (int p = 0; p < 4; ++p) { va[p] = *reinterpret_cast<const f32x4*>(ap[p]); vb[p] = *reinterpret_cast<const f32x4*>(bp[p]); }
    f32x16 acc[2][2];
    for (int m = 0; m < 2; ++m) for (int n = 0; n < 2; ++n) for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.0f;
    float nsq = 0.0f;
    const float (*mine)[kFeatLdsPitch] = tid < FEAT_TILE ? As : Bs;
    const int mrow = tid & (FEAT_TILE - 1);
    const int kh = lane >> 5, l31 = lane & 31;
    for (int k0 = 0; k0 < pitch; k0 += FEAT_KCHUNK) {
        __syncthreads();                                       // the previous chunk's images are consumed
        for (int p = 0; p < 4; ++p)
            for (int c = 0; c < 4; ++c) { As[lc + c][lr + 32 * p] = va[p][c]; Bs[lc + c][lr + 32 * p] = vb[p][c]; }
        __syncthreads();
        if (k0 + FEAT_KCHUNK < pitch)
            for (int p = 0; p < 4; ++p) {
                va[p] = *reinterpret_cast<const f32x4*>(ap[p] + k0 + FEAT_KCHUNK);
                vb[p] = *reinterpret_cast<const f32x4*>(bp[p] + k0 + FEAT_KCHUNK);
            }
#pragma unroll
        for (int k = 0; k < FEAT_KCHUNK; ++k) { const float x = mine[k][mrow]; nsq = fmaf(x, x, nsq); }
#pragma unroll
        for (int kk = 0; kk < FEAT_KCHUNK; kk += 2) {
            const float a0 = As[kk + kh][wr * 64 + l31], a1 = As[kk + kh][wr * 64 + 32 + l31];
            const float b0 = Bs[kk + kh][wc * 64 + l31], b1 = Bs[kk + kh][wc * 64 + 32 + l31];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    nrm[tid] = nsq;
    __syncthreads();
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    double s = 0.0;
    for (int m = 0; m < 2; ++m)
        for (int n = 0; n < 2; ++n) {
            const int lj = wc * 64 + n * 32 + l31;
            const int64_t gj = c0 + lj;
            const float y2 = nrm[FEAT_TILE + lj];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int li = wr * 64 + m * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                const int64_t gi = r0 + li;
                const float dot = acc[m][n][r], x2 = nrm[li];
                float d2 = (x2 - dot) + (y2 - dot);
                d2 = d2 < 0.0f ? 0.0f : d2;
                float v = expm1f((float)(-gamma * (double)d2));
                const bool keep = gi < na && gj < nb && !(same && gi == gj);
                v = keep ? v : 0.0f;
                s += (double)v;
            }
        }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = (double)T.weight * (((wsum[0] + wsum[1]) + wsum[2]) + wsum[3]);
}

// out[0] = the partials added in tile order: thread t adds its run of consecutive tiles in ascending order, thread 0 the 256 run sums in thread order
__global__ __launch_bounds__(256) void feat_pair_sum_kernel(const double* __restrict__ partials, int64_t n, double* __restrict__ out) {
    __shared__ double run[256];
    const int64_t per = (n + 255) / 256, t0 = (int64_t)threadIdx.x * per, t1 = std::min(n, t0 + per);
    double s = 0.0;
    for (int64_t t = t0; t < t1; ++t) s += partials[t];
    run[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double total = run[0];
        for (int t = 1; t < 256; ++t) total += run[t];
        out[0] = total;
    }
}

}  // namespace

}  // namespace tld

using namespace tld;

extern "C" {

int tld_feat_append(float* bank, int64_t capacity, int64_t used, int32_t dim, int32_t pitch, const void* src, int32_t src_dtype, int64_t rows,
                    int32_t normalize, int32_t* bad_count, void* hip_stream) {
    const std::string why = feat_append_check(bank, capacity, used, dim, pitch, src, src_dtype, rows, normalize, bad_count);
    if (!why.empty()) return fail(TLD_ERR_INVALID, "%s", why.c_str());
    if (rows > (int64_t)4 * 0x7fffffff) return fail(TLD_ERR_INVALID, "feat append: rows %lld, more than one launch takes", (long long)rows);
    DeviceGuard dg(std::max(0, ptr_device(bank)));
    hipLaunchKernelGGL(feat_append_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, reinterpret_cast<hipStream_t>(hip_stream), bank, used, (int)dim,
                       (int)pitch, src, (int)src_dtype, rows, (int)normalize, bad_count);
    return check_launch("feat_append_kernel");
}

int tld_feat_moments(const float* bank, int64_t n, int32_t dim, int32_t pitch, double* mean, double* cov, void* hip_stream) {
    const std::string why = feat_moments_check(bank, n, dim, pitch, mean, cov);
    if (!why.empty()) return fail(TLD_ERR_INVALID, "%s", why.c_str());
    if (((uintptr_t)mean & 7) || ((uintptr_t)cov & 7)) return fail(TLD_ERR_INVALID, "feat moments: mean and cov must be 8-byte aligned");
    DeviceGuard dg(std::max(0, ptr_device(bank)));
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const unsigned tiles = (unsigned)((dim + kMomTile - 1) / kMomTile);
    hipLaunchKernelGGL(feat_mean_kernel, dim3(tiles), dim3(64 * kMeanPhases), 0, s, bank, n, (int)dim, (int)pitch, mean);
    if (int rc = check_launch("feat_mean_kernel")) return rc;
    hipLaunchKernelGGL(feat_cov_kernel, dim3(tiles, tiles), dim3(256), 0, s, bank, n, (int)dim, (int)pitch, (const double*)mean, cov);
    return check_launch("feat_cov_kernel");
}

int64_t tld_feat_kernel_sum_partials(int64_t na, int64_t nb, int32_t same) { return feat_tile_count(na, nb, same); }

int tld_feat_kernel_sum(const float* a, int64_t na, const float* b, int64_t nb, int32_t dim, int32_t pitch, double gamma, int32_t same, double* partials,
                        int64_t n_partials, double* out, void* hip_stream) {
    const std::string why = feat_kernel_sum_check(a, na, b, nb, dim, pitch, gamma, same, partials, n_partials, out);
    if (!why.empty()) return fail(TLD_ERR_INVALID, "%s", why.c_str());
    if (((uintptr_t)a & 15) || ((uintptr_t)b & 15)) return fail(TLD_ERR_INVALID, "feat kernel sum: a and b must be 16-byte aligned");
    if (((uintptr_t)partials & 7) || ((uintptr_t)out & 7)) return fail(TLD_ERR_INVALID, "feat kernel sum: partials and out must be 8-byte aligned");
    DeviceGuard dg(std::max(0, ptr_device(a)));
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int64_t tiles = feat_tile_count(na, nb, same);
    hipLaunchKernelGGL(feat_pair_kernel, dim3((unsigned)tiles), dim3(256), 0, s, a, na, b, nb, (int)pitch, gamma, (int)same, partials);
    if (int rc = check_launch("feat_pair_kernel")) return rc;
    hipLaunchKernelGGL(feat_pair_sum_kernel, dim3(1), dim3(256), 0, s, (const double*)partials, tiles, out);
    return check_launch("feat_pair_sum_kernel");
}

}  // extern "C"

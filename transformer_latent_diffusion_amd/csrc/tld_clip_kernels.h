// tld_clip_kernels.h -- what the two CLIP towers (tld_clip.hip: text, tld_clip_vision.hip: image) share: the residual-add + LayerNorm row
// kernels, QuickGELU and the projection helper.  One definition, so both towers compute the same bits.  Include after tld_common.h and tld_host.h;
// the definitions have internal linkage (each tower's translation unit compiles its own copy of the one source).
#pragma once

namespace tld {
namespace {

// One wave per row:  if add: x[row] += add[row] + bias (the residual add of the block that just finished);  out = bf16(LayerNorm(x[row])).
// fp32 statistics, two passes over the row held in registers (W <= 64 * 16).
__global__ __launch_bounds__(256) void clip_add_ln_kernel(float* __restrict__ x, const float* __restrict__ add, const float* __restrict__ bias,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          bf16* __restrict__ out, int T, int W) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= T) return;
    float v[16];
    const int n = W / 64;                          // elements per lane (W % 64 == 0, n <= 16)
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j < n) {
            const int c = j * 64 + lane;
            float f = x[(size_t)row * W + c];
            if (add) { f += add[(size_t)row * W + c] + bias[c]; x[(size_t)row * W + c] = f; }
            v[j] = f; s += f;
        }
    }
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < n) { const float c = v[j] - mean; q = fmaf(c, c, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + kLnEps);
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < n) { const int c = j * 64 + lane; out[(size_t)row * W + c] = (bf16)((v[j] - mean) * rstd * gamma[c] + beta[c]); }
}

// The same for the B pooled rows only (row = b * ctx + eot[b]; eot == nullptr: row b * ctx, the image tower's class token): residual add of the last block, ln_final, fp32 out [B, W]
__global__ __launch_bounds__(64) void clip_final_ln_kernel(const float* __restrict__ x, const float* __restrict__ add, const float* __restrict__ bias,
                                                           const int* __restrict__ eot, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ out, int W, int ctx) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int e = eot ? eot[b] : 0;
    e = e < 0 ? 0 : (e >= ctx ? ctx - 1 : e);
    const size_t row = (size_t)b * ctx + e;
    float v[16];
    const int n = W / 64;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < n) { const int c = j * 64 + lane; v[j] = x[row * W + c] + add[row * W + c] + bias[c]; s += v[j]; }
    const float mean = wave_sum(s) / (float)W;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < n) { const float c = v[j] - mean; q = fmaf(c, c, q); }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)W + kLnEps);
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (j < n) { const int c = j * 64 + lane; out[(size_t)b * W + c] = (v[j] - mean) * rstd * gamma[c] + beta[c]; }
}

// QuickGELU in place: x * sigmoid(1.702 x)      (clip/model.py QuickGELU)
__global__ void clip_quickgelu_kernel(bf16* __restrict__ f, long n8) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n8) return;
    bf16x8 v = *reinterpret_cast<bf16x8*>(f + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (float)v[e];
        v[e] = (bf16)(x * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * x)));
    }
    *reinterpret_cast<bf16x8*>(f + i * 8) = v;
}

// one projection on the persistent MFMA GEMM (tld_gemm.hip): Wt is [N][K] bf16; bias -> bf16 [M, N], or fp32 [M, N] for the two that end in the residual add
int gemm(const bf16* A, int lda, const bf16* Wt, int M, int N, int K, int epi, const float* bias, bf16* out_bf16, float* out_f32, hipStream_t s) {
    GemmParams p{};
    p.A = A; p.lda = lda; p.W = Wt; p.ldw = K; p.M = M; p.N = N; p.K = K; p.bias = bias;
    if (epi == EPI_BIAS_BF16) { p.out_bf16 = out_bf16; p.ldo = N; }
    else { p.c_f32 = out_f32; p.ldc = N; }
    return launch_gemm(p, epi, s);
}

}  // namespace
}  // namespace tld

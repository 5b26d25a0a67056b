// tld_train_attn.hip -- backward of the denoiser's self-attention for the training step.
//
// Forward (tld/transformer_blocks.py:24-48): per (sample, head), O = softmax(Q K^T / 8) V over N tokens, head_dim 64, no mask.
// Backward, given dO:   P = softmax(Q K^T / 8);  dV = P^T dO;  dP = dO V^T;  dS = P o (dP - delta),  delta_q = dO_q . O_q;
//                       dQ = dS K / 8;  dK = dS^T Q / 8.
// A workgroup of NW waves works on blocks of BT = 32 NW tokens: Q, K, dO of a block live in LDS as row-major [BT][64] bf16 (144-byte
// pitch) and V as the forward left it, V^T [64][BT].  Seven BT x BT x 64-class products on v_mfma_f32_32x32x16_bf16, in two passes:
//   pass 1 (a wave owns 32 queries):  S^T = K Q^T and dP^T = V dO^T -- a lane owns a QUERY column, so the softmax statistics and delta are
//           lane-local (+ one lane^32 exchange) -- then dS^T, and dQ^T += K^T dS^T with dS^T going straight from the accumulators into
//           the MFMA's B operand: its 8 values per lane are the keys {(r & 3) + 8 (r >> 2) + 4 hi}, r = 8 s .. 8 s + 7, of the 32-key tile.
//   pass 2 (a wave owns 32 keys):     S = Q K^T and dP = dO V^T (a lane owns a KEY column), P = exp2(S c - L_q) with the row statistics
//           L_q of pass 1, then dV^T += dO^T P and dK^T += Q^T dS the same way.
// Every operand that a product needs TRANSPOSED (K^T, Q^T, dO^T in the accumulators' key / query order; V rows out of V^T) is read
// from the one row-major image with gfx950's transposing LDS read (ds_read_b64_tr_b16: lane i of a 16-lane group receives
// img[k0 + j][m0 + i], j = 0..3, from the 4 x 16 block whose rows the group's lanes address) -- nothing is transposed through memory,
// and no image is kept twice.
//   N <= 256: one workgroup per (sample, head) runs both passes (BT >= N); L and delta stay in LDS.
//   N > 256:  kernel 1, one workgroup per (sample, head, query block): a first sweep over the key blocks for the row statistics,
//           a second for dQ; L and delta go to a scratch vector.  Kernel 2, one workgroup per (sample, head, key block), sweeps the
//           query blocks for dK and dV.
// Any N that is a multiple of 16.  The block width is chosen per N (attn_bwd_block_waves); when N is not a multiple of BT the last query and
// key blocks are partial (the MASKED kernels): rows past N are zero in LDS and never read from memory, keys past N leave the softmax
// (score -inf in pass 1, P = dS = 0 in pass 2), and no dq / dk / dv row or statistic past N is stored.  N % 32 == 16 leaves one 32 x 32
// tile half outside the sample; the masks then act per element, in the accumulator row order.  64, 128, 256 tokens and the multiples of
// 256 keep the unmasked kernels at BT = N (<= 256) or 256.
// Outputs are row-major bf16 [M, 3 d] (dq | dk | dv), the layout the weight- and input-gradient GEMMs consume.
#include "tld_common.h"
#include "tld_train_plan.h"      // attn_bwd_dispatch, attn_bwd_block_waves: which instantiation a token count takes

// attribution builds (tools/attn_bwd_bench.py): -DTLD_AB_DBG=<bits>: 1 no staging loads, 2 no pass 1, 4 no pass 2, 8 no output stores
#ifndef TLD_AB_DBG
#define TLD_AB_DBG 0
#endif

namespace tld {

namespace {

constexpr int kPitch = 144;             // bytes per LDS row of a token-major image: 64 bf16 + 16 B pad
constexpr float kC2 = 0.125f * 1.44269504088896340736f;       // 1/8 scale in log2 units
enum { ATTN_FUSED = 0, ATTN_DQ = 1, ATTN_DKV = 2 };

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

template <int NW> struct Lay {
    static constexpr int BT = 32 * NW;                 // tokens per block
    static constexpr int PV = BT * 2 + 16;             // pitch of the V^T image
    static constexpr int MAT = BT * kPitch;
    static constexpr int Q = 0, K = MAT, G = 2 * MAT, V = 3 * MAT, L = V + 64 * PV, D = L + BT * 4, BYTES = D + BT * 4;
};

__device__ __forceinline__ bf16x8 frag(const char* base, int row, int chunk) {
    return *reinterpret_cast<const bf16x8*>(base + row * kPitch + chunk * 16);
}
// lane i of every 16-lane group: img[k0 + j][m0 + i], j = 0..3 (img row-major bf16, `pitch` bytes per row, m0 a multiple of 4)
__device__ __forceinline__ s16x4 tr4(const char* img, int pitch, int k0, int m0, int lane) {
    const int s = lane & 15;
    const char* p = img + (k0 + (s >> 2)) * pitch + (m0 + 4 * (s & 3)) * 2;
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
}
__device__ __forceinline__ bf16x8 join(s16x4 a, s16x4 b) {
    const s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, v);
}
// MFMA operand (lane = column col0 + l31 of the image): rows row0 + 8 hi + {0 .. 7}
__device__ __forceinline__ bf16x8 tr_seq(const char* img, int pitch, int row0, int col0, int lane) {
    const int m0 = col0 + 16 * ((lane >> 4) & 1), r = row0 + 8 * (lane >> 5);
    return join(tr4(img, pitch, r, m0, lane), tr4(img, pitch, r + 4, m0, lane));
}
// the same with rows row0 + 4 hi + {0 .. 3, 8 .. 11}: the accumulator row order of 16 rows of a 32 x 32 tile
__device__ __forceinline__ bf16x8 tr_acc(const char* img, int pitch, int row0, int col0, int lane) {
    const int m0 = col0 + 16 * ((lane >> 4) & 1), r = row0 + 4 * (lane >> 5);
    return join(tr4(img, pitch, r, m0, lane), tr4(img, pitch, r + 8, m0, lane));
}
__device__ __forceinline__ bf16x8 pack8(const f32x16& a, int s) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (bf16)a[8 * s + e];
    return v;
}
__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    return z;
}
// a 32-token x 64-dim tile held transposed (registers = dims (r & 3) + 8 (r >> 2) + 4 hi of each 32-dim half, lanes = tokens) -> row-major bf16
__device__ __forceinline__ void store_tile(bf16* dst /* row of token l31, first dim */, const f32x16 (&t)[2], float scale, int hi) {
#pragma unroll
    for (int dh = 0; dh < 2; ++dh)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            bf16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (bf16)(t[dh][rq * 4 + e] * scale);
            *reinterpret_cast<bf16x4*>(dst + dh * 32 + 8 * rq + 4 * hi) = v;
        }
}

// TG: dL/dO as fp32 (the test hook) or bf16 (the training step: the LayerNorm-2 backward leaves a bf16 copy of the residual gradient).
// MASKED: N is not a multiple of BT -- the last query / key block is partial (N a multiple of 16, so a 32-token tile is whole, half or empty).
template <int NW, int MODE, typename TG, bool MASKED>
__global__ __launch_bounds__(64 * NW) void attn_bwd_kernel(const bf16* __restrict__ qk, const bf16* __restrict__ vt, const bf16* __restrict__ o,
                                                          const TG* __restrict__ g, bf16* __restrict__ dqkv, float* __restrict__ stats, int H, int N) {
    using Ly = Lay<NW>;
    constexpr int BT = Ly::BT, PV = Ly::PV;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sQ = smem + Ly::Q; char* sK = smem + Ly::K; char* sG = smem + Ly::G; char* sV = smem + Ly::V;
    float* sL = reinterpret_cast<float*>(smem + Ly::L);
    float* sD = reinterpret_cast<float*>(smem + Ly::D);
    const int NB = MASKED ? (N + BT - 1) / BT : N / BT, d = H * 64;
    int bid = blockIdx.x;
    const int blk = bid % NB; bid /= NB;
    const int h = bid % H, b = bid / H;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const size_t row0 = (size_t)b * N;
    float* Lg = stats + ((size_t)(b * H + h) * 2) * N;        // [L | delta] of this (sample, head): only the multi-block kernels touch it
    float* Dg = Lg + N;

    // ---- staging: two threads per token row, four 16-byte chunks each.  MASKED: rows past N are zero in LDS and never read from memory
    // (the zero image keeps the transposing reads, which need every lane, inside the block)
    const int srow = tid >> 1, sc0 = (tid & 1) * 4;
    auto stage_rows = [&](char* img, const bf16* src, int ld, int tb) {
        if (MASKED && tb * BT + srow >= N) {
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<u32x4*>(img + srow * kPitch + (sc0 + c) * 16) = u32x4{0u, 0u, 0u, 0u};
            return;
        }
        const u32x4* p = reinterpret_cast<const u32x4*>(src + (row0 + (size_t)tb * BT + srow) * ld) + sc0;
#pragma unroll
        for (int c = 0; c < 4; ++c) *reinterpret_cast<u32x4*>(img + srow * kPitch + (sc0 + c) * 16) = p[c];
    };
    auto stage_g = [&](int qb, bool with_delta) {          // dO -> bf16 image; delta = dO . O per row
        if (MASKED && qb * BT + srow >= N) {               // dO = 0, delta = 0 (the pair of threads of a row takes this branch together)
#pragma unroll
            for (int c = 0; c < 4; ++c) *reinterpret_cast<u32x4*>(sG + srow * kPitch + (sc0 + c) * 16) = u32x4{0u, 0u, 0u, 0u};
            if (with_delta && (tid & 1) == 0) sD[srow] = 0.f;
            return;
        }
        const size_t row = row0 + (size_t)qb * BT + srow;
        const u32x4* po = reinterpret_cast<const u32x4*>(o + row * d + h * 64) + sc0;
        float delta = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bf16x8 gb;
            float gv[8];
            if constexpr (sizeof(TG) == 4) {
                const float4* pg = reinterpret_cast<const float4*>(g + row * d + h * 64) + sc0 * 2;
                const float4 g0 = pg[2 * c], g1 = pg[2 * c + 1];
                const float t[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) { gv[e] = t[e]; gb[e] = (bf16)t[e]; }
            } else {
                gb = __builtin_bit_cast(bf16x8, (reinterpret_cast<const u32x4*>(g + row * d + h * 64) + sc0)[c]);
#pragma unroll
                for (int e = 0; e < 8; ++e) gv[e] = (float)gb[e];
            }
            if (with_delta) {
                const bf16x8 ob = __builtin_bit_cast(bf16x8, po[c]);
#pragma unroll
                for (int e = 0; e < 8; ++e) delta = fmaf(gv[e], (float)ob[e], delta);
            }
            *reinterpret_cast<bf16x8*>(sG + srow * kPitch + (sc0 + c) * 16) = gb;
        }
        if (with_delta) {
            delta += __shfl_xor(delta, 1, 64);
            if ((tid & 1) == 0) {
                sD[srow] = delta;
                if (MODE == ATTN_DQ) Dg[qb * BT + srow] = delta;
            }
        }
    };
    auto stage_v = [&](int kb) {                           // V^T rows (dims) x BT keys
        constexpr int CPR = BT / 8;                        // 16-byte chunks per row
        const bf16* base = vt + ((size_t)(b * H + h) * 64) * N + (size_t)kb * BT;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int idx = tid + j * 2 * BT, r = idx / CPR, c = idx % CPR;
            if (MASKED && kb * BT + c * 8 >= N) *reinterpret_cast<u32x4*>(sV + r * PV + c * 16) = u32x4{0u, 0u, 0u, 0u};      // (N % 8 == 0: a chunk is whole or past N)
            else *reinterpret_cast<u32x4*>(sV + r * PV + c * 16) = *reinterpret_cast<const u32x4*>(base + (size_t)r * N + c * 8);
        }
    };
    const bf16* qsrc = qk + h * 64;
    const bf16* ksrc = qk + d + h * 64;

    // ================================ pass 1: queries [32 wid, 32 wid + 32) of block `blk` ================================
    if (MODE != ATTN_DKV) {
        if (!(TLD_AB_DBG & 1)) {
            stage_rows(sQ, qsrc, 2 * d, blk);
            stage_g(blk, true);
            if (MODE == ATTN_FUSED) { stage_rows(sK, ksrc, 2 * d, 0); stage_v(0); }
        }
        __syncthreads();
        if (!(TLD_AB_DBG & 2)) {
        const int q0 = 32 * wid;
        bf16x8 qf[4], gf[4];
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) { qf[kc] = frag(sQ, q0 + l31, kc * 2 + hi); gf[kc] = frag(sG, q0 + l31, kc * 2 + hi); }
        const float dlt = sD[q0 + l31];
        f32x16 st[NW];
        auto scores = [&]() {
#pragma unroll
            for (int kt = 0; kt < NW; ++kt) {
                st[kt] = zero16();
#pragma unroll
                for (int kc = 0; kc < 4; ++kc)
                    st[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(sK, kt * 32 + l31, kc * 2 + hi), qf[kc], st[kt], 0, 0, 0);
            }
        };
        // MASKED, last key block kb: scores of keys >= N become -inf before the row statistics and before P in the dQ sweep, so P = 0 there.
        // (A key past N has a zero K row, so a finite dS^T entry would add exactly nothing to dQ -- but its score is 0 and its P = 2^-Lq, which
        // is +inf for a query row whose real scores all lie below -128 in log2 units, and inf x 0 in the dQ product is NaN.)
        auto mask_keys = [&](int kb) {
#pragma unroll
            for (int kt = 0; kt < NW; ++kt) {
                const int lim = N - kb * BT - kt * 32 - 4 * hi;          // (r & 3) + 8 (r >> 2) is the key row of accumulator register r
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if ((r & 3) + 8 * (r >> 2) >= lim) st[kt][r] = -__builtin_inff();
            }
        };
        f32x16 dq[2] = {zero16(), zero16()};
        auto dq_accum = [&]() {                             // st holds P^T of the staged key block
#pragma unroll
            for (int kt = 0; kt < NW; ++kt) {
                f32x16 dp = zero16();
#pragma unroll
                for (int kc = 0; kc < 4; ++kc)
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_seq(sV, PV, 16 * kc, kt * 32, lane), gf[kc], dp, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 16; ++r) dp[r] = st[kt][r] * (dp[r] - dlt);            // dS^T
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const bf16x8 bfrag = pack8(dp, s);
#pragma unroll
                    for (int dh = 0; dh < 2; ++dh)
                        dq[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_acc(sK, kPitch, kt * 32 + 16 * s, dh * 32, lane), bfrag, dq[dh], 0, 0, 0);
                }
            }
        };
        if (MODE == ATTN_FUSED) {
            scores();
            if (MASKED) mask_keys(0);
            float m = -3.0e38f;
#pragma unroll
            for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) m = fmaxf(m, st[kt][r]);
            m = fmaxf(m, __shfl_xor(m, 32, 64)) * kC2;
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) { st[kt][r] = __builtin_amdgcn_exp2f(st[kt][r] * kC2 - m); sum += st[kt][r]; }
            sum += __shfl_xor(sum, 32, 64);
            const float inv = 1.0f / sum;
#pragma unroll
            for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                for (int r = 0; r < 16; ++r) st[kt][r] *= inv;
            if (hi == 0) sL[q0 + l31] = m + __builtin_amdgcn_logf(sum);        // v_log_f32 is log2
            dq_accum();
        } else {
            // sweep 1: row statistics over all key blocks
            float m = -3.0e38f, sum = 0.f;
            for (int kb = 0; kb < NB; ++kb) {
                if (kb) __syncthreads();
                stage_rows(sK, ksrc, 2 * d, kb);
                __syncthreads();
                scores();
                if (MASKED) mask_keys(kb);                   // (a no-op before the last block: there every lim >= 28)
                float mb = -3.0e38f;
#pragma unroll
                for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) mb = fmaxf(mb, st[kt][r]);
                mb = fmaxf(mb, __shfl_xor(mb, 32, 64)) * kC2;
                const float mn = fmaxf(m, mb);
                float part = 0.f;
#pragma unroll
                for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) part += __builtin_amdgcn_exp2f(st[kt][r] * kC2 - mn);
                sum = sum * __builtin_amdgcn_exp2f(m - mn) + part;
                m = mn;
            }
            sum += __shfl_xor(sum, 32, 64);
            const float Lq = m + __builtin_amdgcn_logf(sum);
            if (hi == 0 && (!MASKED || blk * BT + q0 + l31 < N)) Lg[blk * BT + q0 + l31] = Lq;
            // sweep 2: dQ
            for (int kb = 0; kb < NB; ++kb) {
                __syncthreads();
                stage_rows(sK, ksrc, 2 * d, kb);
                stage_v(kb);
                __syncthreads();
                scores();
                if (MASKED && kb == NB - 1) mask_keys(kb);   // P = 0 for keys >= N: their score is 0, and 2^-Lq overflows once Lq < -128
#pragma unroll
                for (int kt = 0; kt < NW; ++kt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[kt][r] = __builtin_amdgcn_exp2f(st[kt][r] * kC2 - Lq);
                dq_accum();
            }
        }
        if (!(TLD_AB_DBG & 8) && (!MASKED || blk * BT + q0 + l31 < N)) store_tile(dqkv + (row0 + (size_t)blk * BT + q0 + l31) * 3 * d + h * 64, dq, 0.125f, hi);
        }
    }
    if (MODE == ATTN_DQ) return;
    if (TLD_AB_DBG & 4) return;

    // ================================ pass 2: keys [32 wid, 32 wid + 32) of block `blk` ================================
    if (MODE == ATTN_DKV) { stage_rows(sK, ksrc, 2 * d, blk); stage_v(blk); }
    __syncthreads();            // FUSED: every query's L is in LDS
    {
        const int k0 = 32 * wid;
        const bool kval = !MASKED || blk * BT + k0 + l31 < N;           // this lane's key lies in the sample
        bf16x8 kf[4], vf[4];
#pragma unroll
        for (int kc = 0; kc < 4; ++kc) { kf[kc] = frag(sK, k0 + l31, kc * 2 + hi); vf[kc] = tr_seq(sV, PV, 16 * kc, k0, lane); }
        f32x16 dk[2] = {zero16(), zero16()}, dv[2] = {zero16(), zero16()};
        for (int qb = 0; qb < NB; ++qb) {
            if (MODE == ATTN_DKV) {
                if (qb) __syncthreads();
                stage_rows(sQ, qsrc, 2 * d, qb);
                stage_g(qb, false);
                if (tid < BT) {
                    if (!MASKED || qb * BT + tid < N) { sL[tid] = Lg[qb * BT + tid]; sD[tid] = Dg[qb * BT + tid]; }
                    else { sL[tid] = 0.f; sD[tid] = 0.f; }      // queries past N: Q = dO = 0, so they add nothing to dK, dV
                }
                __syncthreads();
            }
#pragma unroll NW % 2 ? 1 : 2
            for (int qt = 0; qt < NW; ++qt) {
                f32x16 s = zero16(), dp = zero16();
#pragma unroll
                for (int kc = 0; kc < 4; ++kc) {
                    s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(sQ, qt * 32 + l31, kc * 2 + hi), kf[kc], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag(sG, qt * 32 + l31, kc * 2 + hi), vf[kc], dp, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int qi = qt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    const float p = __builtin_amdgcn_exp2f(s[r] * kC2 - sL[qi]);
                    s[r] = kval ? p : 0.f;                      // P
                    dp[r] = kval ? p * (dp[r] - sD[qi]) : 0.f;  // dS
                }
#pragma unroll
                for (int sl = 0; sl < 2; ++sl) {
                    const bf16x8 pf = pack8(s, sl), dsf = pack8(dp, sl);
#pragma unroll
                    for (int dh = 0; dh < 2; ++dh) {
                        dv[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_acc(sG, kPitch, qt * 32 + 16 * sl, dh * 32, lane), pf, dv[dh], 0, 0, 0);
                        dk[dh] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(tr_acc(sQ, kPitch, qt * 32 + 16 * sl, dh * 32, lane), dsf, dk[dh], 0, 0, 0);
                    }
                }
            }
        }
        bf16* dst = dqkv + (row0 + (size_t)blk * BT + k0 + l31) * 3 * d + h * 64;
        if (!(TLD_AB_DBG & 8) && kval) {
            store_tile(dst + d, dk, 0.125f, hi);
            store_tile(dst + 2 * d, dv, 1.0f, hi);
        }
    }
}

template <int NW, int MODE, typename TG, bool MASKED>
void launch_one(const bf16* qk, const bf16* vt, const bf16* o, const TG* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s) {
    static PerDeviceOnce once;
    once.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_kernel<NW, MODE, TG, MASKED>), hipFuncAttributeMaxDynamicSharedMemorySize, Lay<NW>::BYTES); });
    constexpr int BT = 32 * NW;
    hipLaunchKernelGGL((attn_bwd_kernel<NW, MODE, TG, MASKED>), dim3(batch * heads * ((ntok + BT - 1) / BT)), dim3(64 * NW), Lay<NW>::BYTES, s, qk, vt, o, g, dqkv,
                       stats, heads, ntok);
}

// the instantiation the dispatch chose: returns 4 from the branch that launches a masked kernel, else 0
template <int MODE, typename TG>
int launch_nw(const AttnBwdDispatch& a, const bf16* qk, const bf16* vt, const bf16* o, const TG* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s) {
    int path = 0;
#define TLD_ATTN_BWD_NW(W) \
    case W: \
        if (a.masked) { path = 4; launch_one<W, MODE, TG, true>(qk, vt, o, g, dqkv, stats, batch, ntok, heads, s); } \
        else launch_one<W, MODE, TG, false>(qk, vt, o, g, dqkv, stats, batch, ntok, heads, s); \
        break;
    if constexpr (MODE == ATTN_FUSED) {
        switch (a.waves) { TLD_ATTN_BWD_NW(1) TLD_ATTN_BWD_NW(2) TLD_ATTN_BWD_NW(3) TLD_ATTN_BWD_NW(4) TLD_ATTN_BWD_NW(5) TLD_ATTN_BWD_NW(6) TLD_ATTN_BWD_NW(7)
                           TLD_ATTN_BWD_NW(8) }
    } else {
        switch (a.waves) {
            TLD_ATTN_BWD_NW(4) TLD_ATTN_BWD_NW(5) TLD_ATTN_BWD_NW(6) TLD_ATTN_BWD_NW(8)
            case 7: launch_one<7, MODE, TG, false>(qk, vt, o, g, dqkv, stats, batch, ntok, heads, s); break;      // (exact only: attn_bwd_block_waves picks 7 only where nothing is masked)
        }
    }
#undef TLD_ATTN_BWD_NW
    return path;
}

template <typename TG>
int launch_bwd(const bf16* qk, const bf16* vt, const bf16* o, const TG* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s, int* path_out) {
    const AttnBwdDispatch a = attn_bwd_dispatch(ntok, stats != nullptr);      // (64, 128 and 256 tokens: 2, 4 and 8 waves, exact -- the kernels of the first training engine)
    int path = 0;      // for the stage hook of tld_train.hip: 1 one kernel, 2 two kernels, | 4 masked -- set in the branch that launches
    switch (a.mode) {
    case ATTN_BWD_ONE: path = 1 | launch_nw<ATTN_FUSED>(a, qk, vt, o, g, dqkv, stats, batch, ntok, heads, s); break;
    case ATTN_BWD_TWO:
        path = 2 | launch_nw<ATTN_DQ>(a, qk, vt, o, g, dqkv, stats, batch, ntok, heads, s);
        launch_nw<ATTN_DKV>(a, qk, vt, o, g, dqkv, stats, batch, ntok, heads, s);
        break;
    default: return 1;
    }
    if (path_out) *path_out = path;
    return 0;
}

}  // namespace

// qk [M, 2 d] (q | k) and vt [B, H, 64, N]: the forward's saved operands;  o [M, d]: the forward's output;  g [M, d]: dL/dO (fp32 or bf16);
// dqkv [M, 3 d] bf16 out.  N a multiple of 16 (returns 1 otherwise); `stats` = 2 B H N floats of scratch, touched only when N > 256 (rows < N).
int launch_attention_bwd(const bf16* qk, const bf16* vt, const bf16* o, const float* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s, int* path_out) {
    return launch_bwd<float>(qk, vt, o, g, dqkv, stats, batch, ntok, heads, s, path_out);
}
int launch_attention_bwd(const bf16* qk, const bf16* vt, const bf16* o, const bf16* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s, int* path_out) {
    return launch_bwd<bf16>(qk, vt, o, g, dqkv, stats, batch, ntok, heads, s, path_out);
}

}  // namespace tld

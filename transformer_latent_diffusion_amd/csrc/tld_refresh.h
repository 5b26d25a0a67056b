// tld_refresh.h -- what the inference engine (tld_engine.hip) and its device weight refresh (tld_refresh.hip) share: the per-block weight images of
// an engine and the description of one refresh.  Include after tld_common.h.
#pragma once

#include "tld_param_layout.h"

namespace tld {

// One decoder block's weight images, as tld_engine_finalize_weights allocates them for the engine's mode (a null pointer: not held in this mode).
// Plain pointers only: finalize keeps a device copy of the engine's array of these, and the refresh kernels index it by blockIdx.z.
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

// An image outside the blocks: `n` source elements at flat[src] -> dst
enum { RJ_COPY = 0,          // fp32 [n]
       RJ_SPLIT_HL = 1,      // bf16 [2][n]: hi = bf16(w), lo = bf16(w - float(hi))
       RJ_TRANSPOSE = 2 };   // fp32 [rows][cols] (n = rows * cols) -> [cols][rows]
struct RefreshJob { void* dst; int64_t src, n; int32_t kind, cols; };
constexpr int kRefreshMaxJobs = 24;

struct RefreshPlan {
    int d = 0, hid = 0, L = 0;
    const Layer* layers_dev = nullptr;       // [L]
    LayerOffsets l0{};                       // block 0's offsets in the flat vector; block i: + i * layer_stride
    int64_t layer_stride = 0;
    bool fold = false, fp8 = false;          // any block holds a folded image / the e4m3 images (all blocks of an engine are alike)
    RefreshJob jobs[kRefreshMaxJobs];
    int njobs = 0;
    // out_proj folded into the last block's down projection (tld_tail_fold_math.h); tail_fold_hl null: the engine holds no folded operand
    bf16* tail_fold_hl = nullptr;            // [2][pdp][d + hid] split bf16 image of [Wout | Wout Wd]
    float* tail_fold_b = nullptr;            // [pd] Wout bd + bo
    int64_t outw = 0, outb = 0;              // out_proj weight [pd][d] and bias [pd] in the flat vector
    int pd = 0;
};

// every weight image of the plan from `flat` (fp32, device), enqueued on s: kernels only, no allocation, no synchronisation
int launch_refresh_weights(const RefreshPlan& p, const float* flat, hipStream_t s);
// quant_mx8_host on the device: fp32 [rows][K] -> e4m3 [rows][K] + E8M0 scales [K/128][rows][4]
void launch_quant_mx8_f32(const float* in, uint8_t* out, uint8_t* scale, int rows, int K, hipStream_t s);

}  // namespace tld

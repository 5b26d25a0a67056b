// tld_refresh.h -- what the inference engine (tld_engine.hip) and its device weight refresh (tld_refresh.hip) share: the per-block weight images of
// an engine and the description of one refresh.  Include after tld_common.h.
#pragma once

#include "tld_body_plan.h"        // Layer: one decoder block's weight images
#include "tld_param_layout.h"

namespace tld {

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

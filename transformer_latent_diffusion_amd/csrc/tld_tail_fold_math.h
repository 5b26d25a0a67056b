// tld_tail_fold_math.h -- out_proj folded into the last block's down projection: the arithmetic of the folded
// operand, as refresh_tail_fold_kernel (tld_refresh.hip) builds it; tests/test_tail_fold_host.py holds it on the host against a float64 restatement.
//   W'[f][j] = (float) sum_k double(Wout[f][k]) * double(float(bf16(Wd[k][j])))          [pd x hid]
//   b'[f]    = (float) (sum_k double(Wout[f][k]) * double(bd[k]) + double(bo[f]))
// Sums in double, k = 0 .. d - 1 ascending, one add per element.  A product of two fp32 values is exact in double, so contraction could not change
// a sum; it is pinned off anyway where the compiler knows the pragma.  The image the folded tail kernel reads is [2][pdp][d + hid] bf16: plane 0
// hi = bf16(w), plane 1 lo = bf16(w - float(hi)) of the row [Wout[f] | W'[f]]; rows pd .. pdp - 1 (pdp = patch_dim rounded up to 16) stay zero.
// No HIP in this file: tests/host/tail_fold_main.cpp compiles it on its own.
#pragma once

#include <cstdint>
#include <cstring>

#include "tld_refresh_math.h"

namespace tld {

TLD_HD float tail_fold_f32_from_bits(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
TLD_HD uint32_t tail_fold_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}

// hi | lo halves of one weight
TLD_HD void tail_fold_split(float w, uint16_t* hi, uint16_t* lo) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const uint16_t h = bf16_rne_bits(tail_fold_bits(w));
    *hi = h;
    *lo = bf16_rne_bits(tail_fold_bits(w - tail_fold_f32_from_bits((uint32_t)h << 16)));
}

// W'[f][j]: wout_row = Wout[f] [d], wd = the down projection's fp32 weight [d][hid]
TLD_HD float tail_fold_weight(const float* wout_row, const float* wd, int d, int hid, int j) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int k = 0; k < d; ++k) {
        const float q = tail_fold_f32_from_bits((uint32_t)bf16_rne_bits(tail_fold_bits(wd[(int64_t)k * hid + j])) << 16);
        s += (double)wout_row[k] * (double)q;
    }
    return (float)s;
}

// b'[f]
TLD_HD float tail_fold_bias(const float* wout_row, const float* bd, float bo, int d) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int k = 0; k < d; ++k) s += (double)wout_row[k] * (double)bd[k];
    return (float)(s + (double)bo);
}

TLD_HD int tail_fold_padded_rows(int pd) { return (pd + 15) / 16 * 16; }

}  // namespace tld

// tld_normal_device.h -- device half of the generator of tld_batch_math.h: Philox words to standard normals, for the kernels that draw them
// (prepare_batch_kernel in tld_batch.hip, sampler_step_kernel<.., NOISE> and sampler_noise_debug_kernel in tld_rows.hip).  HIP device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "tld_batch_math.h"

namespace tld {

// ln of the unrounded u = ((r >> 8) + 0.5) 2^-24: u is exact in fp32 below one half, 1 - u is exact from there on
__device__ __forceinline__ float log_uniform24_open(uint32_t r) {
    return (r >> 8) < 0x800000u ? logf(uniform24_open(r)) : log1pf(-uniform24_open_complement(r));
}

// the four normals of one counter: two Box-Muller pairs, (v[0], v[1]) -> n[0], n[1] and (v[2], v[3]) -> n[2], n[3]; the loop of prepare_batch_kernel
__device__ __forceinline__ void philox_normals4(const Philox4& p, float n[4]) {
#pragma clang fp contract(off)
    for (int h = 0; h < 2; ++h) {
        const float rad = __fsqrt_rn(-2.f * log_uniform24_open(p.v[2 * h]));
        float sn, cs;
        sincospif(2.f * uniform24_open(p.v[2 * h + 1]), &sn, &cs);
        n[2 * h] = rad * cs;
        n[2 * h + 1] = rad * sn;
    }
}

}  // namespace tld

// tld_sampler_noise.h -- where the stochastic sampler's noise comes from (tld_sample_requests_stochastic): the Philox counter of
// one draw, in plain integer arithmetic on top of tld_batch_math.h.  No HIP in this file: tests/host/sampler_noise_main.cpp compiles it on its own
// and tests/stochastic_ref.py restates it in numpy.
//
// Four consecutive elements of a request's image share one counter, as in prepare_batch_kernel:
//   counter = (quad, step, SAMPLER_NOISE_TAG, 0)      quad = (element index inside the request's own [C, S, S] image) / 4
//                                                     step = forward index i of the request's own trajectory (0 = its first forward)
//   key     = the request's 64-bit noise key (low word, high word)
// Nothing about the request's place in the batch, the number of requests running or the rank enters it: a request alone and the same request in a mixed
// call read the same words.  The four words become two Box-Muller pairs, elements 4 quad + {0, 1} from (v[0], v[1]) and 4 quad + {2, 3} from (v[2], v[3])
// (tld_normal_device.h).  The tag names the stream: under an equal key the batch preparation (whose third word is the low half of its step counter) meets
// these counters only at training step 0x534E5A31.
#pragma once

#include "tld_batch_math.h"

namespace tld {

constexpr uint32_t SAMPLER_NOISE_TAG = 0x534E5A31u;      // "SNZ1"

TLD_HD Philox4 sampler_noise_philox(uint64_t key, uint32_t step, uint32_t quad) {
    return philox4x32_10(quad, step, SAMPLER_NOISE_TAG, 0u, (uint32_t)key, (uint32_t)(key >> 32));
}

}  // namespace tld

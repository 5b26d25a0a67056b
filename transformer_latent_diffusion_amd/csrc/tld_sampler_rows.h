// tld_sampler_rows.h -- the rows of the sampler's one staged upload, as the host writes them (tld_sample_plan.h) and the step kernel reads them
// (tld_common.h, tld_rows.hip).  No HIP in this file.
#pragma once

#include <cstdint>

namespace tld {

// what differs per sample in the elementwise step, one row per (step, request), or one per step shared by every sample
struct SamplerStepRow {
    float g, a, b, c, c1, c2;     // class guidance and the step's coefficients of the request (schedule.py)
    float s_next;                 // noise level the updated x_t sits at (read with a mask only; unused on the request's final step)
    int final_step;               // 1: the request's last level -- combine (+ mask blend, + shifts on channels 3 and 0) into out_latent, no update
                                  // (the slots flavour packs final | (slot + 1) << 1 here: see launch_sampler_step)
};
static_assert(sizeof(SamplerStepRow) == 32, "eight 4-byte fields, no padding: the upload is compared byte for byte");
// second table of the stochastic entry, one row per (step, request) beside SamplerStepRow: x_t += e z after the update, z the standard normals of
// (key, step, quad) (tld_sampler_noise.h).  e == 0.0f: nothing is drawn and nothing is added
struct alignas(16) SamplerNoiseRow {
    float e;                      // sigma_t sqrt(1 - exp(-2 eta h)) of the request's step (schedule.py); 0 on its final forward
    uint32_t key_lo, key_hi;      // the request's 64-bit noise key
    uint32_t reserved;
};
static_assert(sizeof(SamplerNoiseRow) == 16, "one 16-byte row");

}  // namespace tld

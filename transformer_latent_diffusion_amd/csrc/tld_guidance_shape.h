// tld_guidance_shape.h -- the shape of the guidance update (tld_sample_requests_shaped): guidance rescale (Lin et al. 2023)
// and adaptive projected guidance, APG (Sadat et al. 2024), as one pair of fp32 weights (P, Q) per request and forward, made in double from five sums
// over the request's image.  No HIP in this file: tests/host/guidance_shape_main.cpp compiles it on its own and tests/shaped_ref.py restates it in numpy.
//
// c the conditional prediction, u the unconditional one, n elements, g the forward's guidance, m the request's momentum buffer:
//   d    = fl32(c - u)                                dbar = beta != 0 ? fl32(d + fl32(beta m)) : d          then m <- dbar
//   Sc = sum c   Sd = sum dbar   Scc = sum c^2   Sdc = sum dbar c   Sdd = sum dbar^2                          in double
//   s    = (norm_r > 0 && Sdd > 0) ? min(1, norm_r / sqrt(Sdd)) : 1                                           the update clipped to norm r
//   p    = Scc > 0 ? s Sdc / Scc : 0                                                                          its part along c
//   A    = 1 + (g - 1)(eta_par - 1) p      B = (g - 1) s          x_apg = A c + B dbar = c + (g - 1)(d_orth + eta_par d_par)
//   vc   = Scc - Sc^2 / n                  vx = A^2 Scc + 2 A B Sdc + B^2 Sdd - (A Sc + B Sd)^2 / n          n var(c), n var(x_apg)
//   k    = (phi != 0 && vc > 0 && vx > 0) ? phi sqrt(vc / vx) + (1 - phi) : 1                                 the rescale
//   P    = fl32(k A)      Q = fl32(k B)                                                                       x0 = fma(P, c, fl32(Q dbar))
#pragma once

#include <cmath>

#include "tld_batch_math.h"      // TLD_HD

namespace tld {

// one row per request: the four values of the C entry, in its order
struct alignas(16) GuidanceShape {
    float eta_par;               // weight of the update's part parallel to c; 1: off
    float norm_r;                // the update's norm is clipped to it; 0: off
    float beta;                  // momentum over the updates (APG uses negative values); 0: off
    float phi;                   // guidance rescale; 0: off
    // all four off: the request takes plain CFG, fma(g, c, (1 - g) u)
    TLD_HD bool neutral() const { return eta_par == 1.0f && norm_r == 0.0f && beta == 0.0f && phi == 0.0f; }
};
static_assert(sizeof(GuidanceShape) == 16, "GuidanceShape is the C entry's row of four floats");

enum { GS_SC = 0, GS_SD = 1, GS_SCC = 2, GS_SDC = 3, GS_SDD = 4, GS_SUMS = 5 };

struct GuidanceWeights { float P, Q; };

// (sums, n, g, shape) -> (P, Q): double until the two final roundings, every operation rounded on its own
TLD_HD GuidanceWeights guidance_shape_finalize(const double sums[GS_SUMS], int n, float g, const GuidanceShape& h) {
#pragma clang fp contract(off)
    const double Sc = sums[GS_SC], Sd = sums[GS_SD], Scc = sums[GS_SCC], Sdc = sums[GS_SDC], Sdd = sums[GS_SDD];
    const double gm1 = (double)g - 1.0, nn = (double)n;
    double s = 1.0;
    if (h.norm_r > 0.0f && Sdd > 0.0) {
        const double q = (double)h.norm_r / sqrt(Sdd);
        s = q < 1.0 ? q : 1.0;
    }
    const double p = Scc > 0.0 ? s * Sdc / Scc : 0.0;
    const double A = 1.0 + gm1 * ((double)h.eta_par - 1.0) * p;
    const double B = gm1 * s;
    double k = 1.0;
    if (h.phi != 0.0f) {
        const double vc = Scc - Sc * Sc / nn;
        const double mx = A * Sc + B * Sd;
        const double vx = A * A * Scc + 2.0 * A * B * Sdc + B * B * Sdd - mx * mx / nn;
        if (vc > 0.0 && vx > 0.0) k = (double)h.phi * sqrt(vc / vx) + (1.0 - (double)h.phi);
    }
    return GuidanceWeights{(float)(k * A), (float)(k * B)};
}

// the values the C entries refuse: non-finite, eta_par < 0, norm_r < 0, |beta| >= 1, phi outside [0, 1].  Returns the name of the first bad field, or null
inline const char* guidance_shape_invalid(const GuidanceShape& h) {
    if (!(std::isfinite(h.eta_par) && h.eta_par >= 0.0f)) return "eta_par (expected finite and >= 0)";
    if (!(std::isfinite(h.norm_r) && h.norm_r >= 0.0f)) return "norm_r (expected finite and >= 0)";
    if (!(std::isfinite(h.beta) && std::fabs(h.beta) < 1.0f)) return "beta (expected |beta| < 1)";
    if (!(std::isfinite(h.phi) && h.phi >= 0.0f && h.phi <= 1.0f)) return "phi (expected inside [0, 1])";
    return nullptr;
}

}  // namespace tld

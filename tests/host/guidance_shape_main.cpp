// Host driver for csrc/tld_guidance_shape.h: the finalisation of the shaped guidance update compiled by the host compiler alone.
// guidance_shape_main (<n> <g> <eta_par> <norm_r> <beta> <phi> <Sc> <Sd> <Scc> <Sdc> <Sdd>)...  -> per group of eleven arguments one line
//     P Q neutral invalid
// n in decimal, the five floats and the five double sums as bit patterns in hex; P and Q come back as fp32 bit patterns in hex, `neutral` is the row's
// predicate and `invalid` 1 where the C entries would refuse the row.  tests/test_guidance_shape_host.py compares P and Q with tests/shaped_ref.py,
// bit for bit; it builds this file with -ffp-contract=off, plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tld_guidance_shape.h"

static float f32(const char* hex) {
    const uint32_t u = (uint32_t)std::strtoul(hex, nullptr, 16);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

static double f64(const char* hex) {
    const uint64_t u = std::strtoull(hex, nullptr, 16);
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc < 12 || (argc - 1) % 11 != 0) {
        std::fprintf(stderr, "usage: %s (<n> <g> <eta_par> <norm_r> <beta> <phi> <Sc> <Sd> <Scc> <Sdc> <Sdd>)...\n", argv[0]);
        return 2;
    }
    const int cases = (argc - 1) / 11;
    std::vector<tld::GuidanceWeights> out((size_t)cases);
    std::vector<int> flags((size_t)cases);
    for (int k = 0; k < cases; ++k) {
        char** a = argv + 1 + 11 * k;
        const int n = (int)std::strtol(a[0], nullptr, 10);
        if (n <= 0) return 2;
        const float g = f32(a[1]);
        const tld::GuidanceShape h{f32(a[2]), f32(a[3]), f32(a[4]), f32(a[5])};
        double sums[tld::GS_SUMS];
        for (int j = 0; j < tld::GS_SUMS; ++j) sums[j] = f64(a[6 + j]);
        out[(size_t)k] = tld::guidance_shape_finalize(sums, n, g, h);
        flags[(size_t)k] = (h.neutral() ? 1 : 0) | (tld::guidance_shape_invalid(h) ? 2 : 0);
    }
    for (int k = 0; k < cases; ++k)
        std::printf("%08x %08x %d %d\n", bits(out[(size_t)k].P), bits(out[(size_t)k].Q), flags[(size_t)k] & 1, flags[(size_t)k] >> 1);
    return 0;
}

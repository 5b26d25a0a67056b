// Host driver for csrc/tld_sampler_noise.h: the counter layout of the stochastic sampler's noise compiled by the host compiler alone.
// sampler_noise_main <key> <step> <first_quad> <n>  -> for quad = first_quad .. first_quad + n - 1 one line
//     quad  w0 w1 w2 w3  u_open(w0..w3)  u_open_complement(w0..w3)
// the Philox words in hex and the two fp32 uniforms the normals are made of as bit patterns in hex.  tests/test_stochastic_host.py compares every
// field with tests/stochastic_ref.py, bit for bit; it builds this file plain and with -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tld_sampler_noise.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 5) {
        std::fprintf(stderr, "usage: %s <key> <step> <first_quad> <n>\n", argv[0]);
        return 2;
    }
    const uint64_t key = std::strtoull(argv[1], nullptr, 0);
    const uint32_t step = (uint32_t)std::strtoul(argv[2], nullptr, 0);
    const uint64_t first = std::strtoull(argv[3], nullptr, 0);
    const long n = std::strtol(argv[4], nullptr, 0);
    if (n <= 0 || first + (uint64_t)n > (1ull << 32)) return 2;
    std::vector<tld::Philox4> words((size_t)n);
    for (long q = 0; q < n; ++q) words[(size_t)q] = tld::sampler_noise_philox(key, step, (uint32_t)(first + (uint64_t)q));
    for (long q = 0; q < n; ++q) {
        const tld::Philox4& p = words[(size_t)q];
        std::printf("%" PRIu64 " %08x %08x %08x %08x", first + (uint64_t)q, p.v[0], p.v[1], p.v[2], p.v[3]);
        for (int k = 0; k < 4; ++k) std::printf(" %08x", bits(tld::uniform24_open(p.v[k])));
        for (int k = 0; k < 4; ++k) std::printf(" %08x", bits(tld::uniform24_open_complement(p.v[k])));
        std::printf("\n");
    }
    return 0;
}

// Host driver for csrc/tld_attn_vimage.h -- the row-major LDS image of V of the fused QKV + attention epilogues, its transposing read and the LDS map of the
// two-head epilogue (tests/test_attn_vimage_host.py; built plain and with -fsanitize=address,undefined).  The image is filled through the write map with
// the code key * 64 + feature, the transposing read (ds_read_b64_tr_b16) is emulated from its lane map, and every (lane, step, feature tile, read) is held
// to the operand order attn256_wave needs, to 8-byte alignment and to the bank rules.
//
//   attn_vimage_main check     every check; prints "OK <n> reads" and exits 0, or the first failures and exits 1
//   attn_vimage_main map       the regions of the two phases of the pair LDS map, one per line: phase name begin end
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tld_attn_vimage.h"

using namespace tld;

static int fails = 0;
#define FAIL(...) do { if (fails++ < 20) { std::printf("FAIL: " __VA_ARGS__); std::printf("\n"); } } while (0)

// One wave-level 8-byte store of a register quad: lane = (l31, hi) writes features f0 + 4 hi .. + 3 of row r0 + l31.
// cols = features per wave column: 32 in the one-head form (4 quads), 16 in the pair form (2 quads).
static void fill(std::vector<uint16_t>& img, std::vector<int>& hits, int cols) {
    for (int wn = 0; wn < 64 / cols; ++wn)
        for (int rq = 0; rq < cols / 8; ++rq)
            for (int r0 = 0; r0 < 256; r0 += 32) {
                int bank[32] = {};
                for (int lane = 0; lane < 64; ++lane) {
                    const int row = r0 + (lane & 31), f = wn * cols + 8 * rq + 4 * (lane >> 5);
                    const int a = attn_v_off(row, f);
                    if (a % 8 || a < 0 || a + 8 > kAttnVImageBytes) { FAIL("write address %d of row %d feature %d", a, row, f); continue; }
                    for (int e = 0; e < 4; ++e) { img[a / 2 + e] = (uint16_t)(row * 64 + f + e); ++hits[a / 2 + e]; }
                    ++bank[(a / 4) % 32]; ++bank[(a / 4 + 1) % 32];
                }
                for (int b = 0; b < 32; ++b)
                    if (bank[b] > 4) FAIL("write (cols %d, wn %d, rq %d, rows %d..): bank %d is hit by %d lanes", cols, wn, rq, r0, b, bank[b]);
            }
}

static int check() {
    long reads = 0;
    for (int cols : {32, 16}) {
        std::vector<uint16_t> img(kAttnVImageBytes / 2, 0xFFFF);
        std::vector<int> hits(kAttnVImageBytes / 2, 0);
        fill(img, hits, cols);
        for (size_t k = 0; k < hits.size(); ++k)
            if (hits[k] != 1) FAIL("cols %d: element at byte %zu written %d times", cols, 2 * k, hits[k]);
        for (int s2 = 0; s2 < 16; ++s2)
            for (int ct = 0; ct < 2; ++ct)
                for (int rd = 0; rd < 2; ++rd) {
                    int addr[64];
                    for (int lane = 0; lane < 64; ++lane) {
                        addr[lane] = attn_v_tr_step(attn_v_tr_addr(lane, 0, 0, 0), s2, ct, rd);        // the kernel's form: one base per lane
                        if (addr[lane] != attn_v_tr_addr(lane, s2, ct, rd)) FAIL("tr_step != tr_addr at lane %d s2 %d ct %d rd %d", lane, s2, ct, rd);
                        if (addr[lane] % 8 || addr[lane] < 0 || addr[lane] + 8 > kAttnVImageBytes) FAIL("read address %d at lane %d s2 %d ct %d rd %d", addr[lane], lane, s2, ct, rd);
                    }
                    for (int half = 0; half < 2; ++half) {         // 64 banks of 4 bytes per 32-lane half, every one exactly once
                        int bank[64] = {};
                        for (int l = 0; l < 32; ++l) { ++bank[(addr[half * 32 + l] / 4) % 64]; ++bank[(addr[half * 32 + l] / 4 + 1) % 64]; }
                        for (int b = 0; b < 64; ++b)
                            if (bank[b] != 1) FAIL("read s2 %d ct %d rd %d half %d: bank %d is hit %d times", s2, ct, rd, half, b, bank[b]);
                    }
                    // the gather: per group of 16 lanes, lane 4q + p supplies row q, columns 4p .. 4p + 3; lane i receives column i, row q in element q
                    for (int lane = 0; lane < 64; ++lane) {
                        const int grp = lane & ~15, i = lane & 15, l31 = lane & 31, hi = lane >> 5;
                        for (int q = 0; q < 4; ++q) {
                            const int src = addr[grp + 4 * q + (i >> 2)] + 2 * (i & 3);
                            const int got = img[src / 2], want = (16 * s2 + 8 * rd + 4 * hi + q) * 64 + 32 * ct + l31;
                            if (got != want)
                                FAIL("cols %d lane %d s2 %d ct %d rd %d element %d: key %d feature %d, want key %d feature %d", cols, lane, s2, ct, rd, q, got / 64, got % 64,
                                     want / 64, want % 64);
                        }
                        ++reads;
                    }
                }
    }
    // the LDS map of the two-head epilogue: the regions of each phase are disjoint and inside the CU's 160 KiB
    if (!pair_regions_ok(kPairPhase1)) FAIL("pair LDS map, phase 1 (correction: tables + four images)");
    if (!pair_regions_ok(kPairPhase2)) FAIL("pair LDS map, phase 2 (attention: five images)");
    for (const PairRegion& r : kPairPhase1) if (r.end > 163840) FAIL("%s ends at %d", r.name, r.end);
    for (const PairRegion& r : kPairPhase2) if (r.end > 163840) FAIL("%s ends at %d", r.name, r.end);
    if (fails) { std::printf("%d failures\n", fails); return 1; }
    std::printf("OK %ld reads\n", reads);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "check")) return check();
    if (argc == 2 && !std::strcmp(argv[1], "map")) {
        for (const PairRegion& r : kPairPhase1) std::printf("1 %s %d %d\n", r.name, r.begin, r.end);
        for (const PairRegion& r : kPairPhase2) std::printf("2 %s %d %d\n", r.name, r.begin, r.end);
        return 0;
    }
    std::fprintf(stderr, "usage: attn_vimage_main check | map\n");
    return 2;
}

// Stand-alone check of csrc/tld_feat_plan.h (the ordered tile list of the all-pairs kernel sum and the argument checks of the tld_feat_* entry points),
// built by tests/test_metrics_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     feat_plan_main CASES.txt        one case per line: "na nb same"
//
// For every case it lays the tiles over an na x nb count matrix -- a tile of weight 2 also over its mirror image -- and checks that every (i, j) is
// covered exactly once, that no tile is empty or reaches past the last row block, that the count equals feat_tile_count and that feat_tile_at agrees
// with the list; then it prints
//     na nb same n_tiles  ti tj w  ti tj w ...
// which tests/metrics_ref.py restates.  A broken property prints the case and makes the exit status 1.
#include "tld_feat_plan.h"

#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>

using namespace tld;

static int check_case(int64_t na, int64_t nb, int32_t same) {
    auto bad = [&](const char* what, long long at) { std::printf("%lld %lld %d: BROKEN %s at %lld\n", (long long)na, (long long)nb, same, what, at); return 1; };
    const std::vector<FeatTile> tiles = feat_plan(na, nb, same);
    if ((int64_t)tiles.size() != feat_tile_count(na, nb, same)) return bad("tile count", (long long)tiles.size());
    std::vector<int32_t> cover((size_t)(na * nb), 0);
    for (size_t t = 0; t < tiles.size(); ++t) {
        const FeatTile k = tiles[t], again = feat_tile_at((int64_t)t, na, nb, same);
        if (again.ti != k.ti || again.tj != k.tj || again.weight != k.weight) return bad("feat_tile_at", (long long)t);
        const int64_t i0 = (int64_t)k.ti * FEAT_TILE, j0 = (int64_t)k.tj * FEAT_TILE;
        if (k.ti < 0 || k.tj < 0 || i0 >= na || j0 >= nb) return bad("empty tile", (long long)t);
        if (k.weight != 1 && k.weight != 2) return bad("weight", (long long)t);
        if (k.weight == 2 && (!same || k.ti == k.tj)) return bad("doubled tile", (long long)t);
        if (same && k.tj < k.ti) return bad("tile below the diagonal", (long long)t);
        for (int64_t i = i0; i < i0 + FEAT_TILE && i < na; ++i)
            for (int64_t j = j0; j < j0 + FEAT_TILE && j < nb; ++j) {
                ++cover[(size_t)(i * nb + j)];
                if (k.weight == 2) ++cover[(size_t)(j * nb + i)];          // the mirror image (same = 1: na == nb)
            }
    }
    for (int64_t p = 0; p < na * nb; ++p)
        if (cover[(size_t)p] != 1) return bad("pair not covered exactly once", (long long)p);
    std::printf("%" PRId64 " %" PRId64 " %d %zu", na, nb, same, tiles.size());
    for (const FeatTile& k : tiles) std::printf("  %d %d %d", k.ti, k.tj, k.weight);
    std::printf("\n");
    return 0;
}

// the refusals, each by its text
static int check_refusals() {
    int fails = 0;
    auto expect = [&fails](const std::string& got, const char* want) {
        const bool ok = *want ? got.find(want) != std::string::npos : got.empty();
        if (!ok) { std::printf("refusal: wanted '%s', got '%s'\n", want, got.c_str()); ++fails; }
    };
    float a[64], b[64];
    double p[4], out;
    int32_t badc;
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 32, 0.005, 0, p, 1, &out), "");
    expect(feat_kernel_sum_check(a, 2, a, 2, 8, 32, 0.0, 1, p, 1, &out), "");
    expect(feat_kernel_sum_check(nullptr, 2, b, 2, 8, 32, 0.005, 0, p, 1, &out), "a is NULL");
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 32, 0.005, 0, nullptr, 1, &out), "partials is NULL");
    expect(feat_kernel_sum_check(a, 2, b, 2, 0, 32, 0.005, 0, p, 1, &out), "dim 0 outside");
    expect(feat_kernel_sum_check(a, 2, b, 2, 4097, 4128, 0.005, 0, p, 1, &out), "dim 4097 outside");
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 8, 0.005, 0, p, 1, &out), "pitch 8 is not dim rounded up");
    expect(feat_kernel_sum_check(a, 0, b, 2, 8, 32, 0.005, 0, p, 1, &out), "na 0, nb 2");
    expect(feat_kernel_sum_check(a, 2, a, 3, 8, 32, 0.005, 1, p, 1, &out), "same = 1 with na 2 != nb 3");
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 32, 0.005, 1, p, 1, &out), "same = 1 with a != b");
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 32, -1.0, 0, p, 1, &out), "gamma -1");
    expect(feat_kernel_sum_check(a, 2, b, 2, 8, 32, std::numeric_limits<double>::quiet_NaN(), 0, p, 1, &out), "gamma nan");
    expect(feat_kernel_sum_check(a, 129, b, 129, 8, 32, 0.005, 0, p, 3, &out), "partials holds 3 doubles, the plan needs 4");
    expect(feat_append_check(a, 2, 0, 8, 32, b, 0, 2, 1, &badc), "");
    expect(feat_append_check(a, 2, 1, 8, 32, b, 0, 2, 1, &badc), "do not fit a bank of 2 rows");
    expect(feat_append_check(a, 2, 0, 8, 32, b, 3, 2, 1, &badc), "src_dtype 3");
    expect(feat_append_check(a, 2, 0, 8, 32, b, 0, 0, 1, &badc), "rows 0");
    expect(feat_moments_check(a, 2, 8, 32, p, p), "");
    expect(feat_moments_check(a, 1, 8, 32, p, p), "n 1");
    if (feat_pitch(1) != 32 || feat_pitch(32) != 32 || feat_pitch(33) != 64 || feat_pitch(4096) != 4096) { std::printf("feat_pitch\n"); ++fails; }
    if (feat_tile_count(0, 5, 0) != 0 || feat_tile_count(5, 6, 1) != 0) { std::printf("feat_tile_count of refused sizes\n"); ++fails; }
    return fails;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    std::ifstream in(argv[1]);
    if (!in) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    int fails = check_refusals();
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        long long na, nb; int same;
        if (!(ls >> na >> nb >> same)) continue;
        if (na < 1 || nb < 1 || na * nb > (1 << 22)) { std::printf("%s: outside what this program lays out\n", line.c_str()); ++fails; continue; }
        fails += check_case(na, nb, same);
    }
    std::printf("tile %d %d failures\n", FEAT_TILE, fails);
    return fails ? 1 : 0;
}

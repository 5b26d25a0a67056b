// tld_feat_plan.h -- the work list of the all-pairs kernel sum (tld_metrics.hip: tld_feat_kernel_sum): a pure function from
// (na, nb, same) to the ordered list of 128 x 128 tiles the pair kernel takes one workgroup each, and the argument checks of the three tld_feat_*
// entry points.  No HIP in this file: tests/host/feat_plan_main.cpp compiles it with the host compiler alone and tests/metrics_ref.py restates the cut.
//
// The cut: rows of `a` in blocks of FEAT_TILE, rows of `b` in blocks of FEAT_TILE.  same = 0: every (ti, tj), ti-major, weight 1.  same = 1 (b is a,
// the pair matrix is symmetric): only tj >= ti, ti-major; a tile off the diagonal stands for its mirror image too and has weight 2, a diagonal tile
// has weight 1 and the kernel drops its i == j terms.  Tile t writes partials[t]; the final sum adds the partials in this order.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define TLD_FEAT_HD __host__ __device__
#else
#define TLD_FEAT_HD
#endif

namespace tld {

constexpr int32_t FEAT_TILE = 128;                         // rows of a and rows of b per workgroup
constexpr int32_t FEAT_KCHUNK = 32;                        // columns per LDS stage; the bank's pitch is a multiple of it
constexpr int32_t FEAT_MAX_DIM = 4096;
constexpr int64_t FEAT_MAX_TILES = 0x7fffffff;             // one workgroup per tile on grid.x

struct FeatTile { int32_t ti, tj, weight; };               // rows [128 ti, 128 ti + 128) of a against rows [128 tj, 128 tj + 128) of b

TLD_FEAT_HD inline int64_t feat_pitch(int64_t dim) { return (dim + FEAT_KCHUNK - 1) / FEAT_KCHUNK * FEAT_KCHUNK; }
TLD_FEAT_HD inline int64_t feat_row_tiles(int64_t n) { return (n + FEAT_TILE - 1) / FEAT_TILE; }

// tiles of the whole list (0 when the sizes are refused)
TLD_FEAT_HD inline int64_t feat_tile_count(int64_t na, int64_t nb, int32_t same) {
    if (na < 1 || nb < 1 || (same && na != nb)) return 0;
    const int64_t ta = feat_row_tiles(na), tb = feat_row_tiles(nb);
    return same ? ta * (ta + 1) / 2 : ta * tb;
}

// tile t of the list; 0 <= t < feat_tile_count.  (same = 1: row ti of the triangle starts at ti ta - ti (ti - 1) / 2.)
TLD_FEAT_HD inline FeatTile feat_tile_at(int64_t t, int64_t na, int64_t nb, int32_t same) {
    const int64_t ta = feat_row_tiles(na), tb = feat_row_tiles(nb);
    if (!same) return FeatTile{(int32_t)(t / tb), (int32_t)(t % tb), 1};
    int64_t ti = 0, start = 0;
    while (start + (ta - ti) <= t) { start += ta - ti; ++ti; }
    const int64_t tj = ti + (t - start);
    return FeatTile{(int32_t)ti, (int32_t)tj, tj == ti ? 1 : 2};
}

inline std::vector<FeatTile> feat_plan(int64_t na, int64_t nb, int32_t same) {
    const int64_t n = feat_tile_count(na, nb, same);
    std::vector<FeatTile> tiles;
    tiles.reserve((size_t)n);
    for (int64_t t = 0; t < n; ++t) tiles.push_back(feat_tile_at(t, na, nb, same));
    return tiles;
}

namespace feat_detail {
inline std::string say(const char* fmt, long long a, long long b) { char s[200]; std::snprintf(s, sizeof s, fmt, a, b); return std::string(s); }
inline std::string check_width(const char* who, int64_t dim, int64_t pitch) {
    if (dim < 1 || dim > FEAT_MAX_DIM) return std::string(who) + say(": dim %lld outside [1, %lld]", (long long)dim, (long long)FEAT_MAX_DIM);
    if (pitch != feat_pitch(dim)) return std::string(who) + say(": pitch %lld is not dim rounded up to a multiple of 32 (%lld)", (long long)pitch, (long long)feat_pitch(dim));
    return std::string();
}
}  // namespace feat_detail

// The refusals of tld_feat_kernel_sum, in the order of include/tld_hip.h; "" when the arguments are good.
inline std::string feat_kernel_sum_check(const void* a, int64_t na, const void* b, int64_t nb, int64_t dim, int64_t pitch, double gamma, int32_t same,
                                         const void* partials, int64_t n_partials, const void* out) {
    using namespace feat_detail;
    const char* who = "feat kernel sum";
    if (!a) return std::string(who) + ": a is NULL";
    if (!b) return std::string(who) + ": b is NULL";
    if (!partials) return std::string(who) + ": partials is NULL";
    if (!out) return std::string(who) + ": out is NULL";
    const std::string w = check_width(who, dim, pitch);
    if (!w.empty()) return w;
    if (na < 1 || nb < 1) return std::string(who) + say(": na %lld, nb %lld (at least one row each)", (long long)na, (long long)nb);
    if (same != 0 && same != 1) return std::string(who) + say(": same %lld (0 or 1)", same, 0);
    if (same && na != nb) return std::string(who) + say(": same = 1 with na %lld != nb %lld", (long long)na, (long long)nb);
    if (same && a != b) return std::string(who) + ": same = 1 with a != b";
    if (!std::isfinite(gamma) || gamma < 0.0) { char s[120]; std::snprintf(s, sizeof s, ": gamma %g (finite and >= 0)", gamma); return std::string(who) + s; }
    const int64_t tiles = feat_tile_count(na, nb, same);
    if (tiles > FEAT_MAX_TILES) return std::string(who) + say(": %lld tiles, more than one launch takes (%lld)", (long long)tiles, (long long)FEAT_MAX_TILES);
    if (n_partials < tiles) return std::string(who) + say(": partials holds %lld doubles, the plan needs %lld", (long long)n_partials, (long long)tiles);
    return std::string();
}

// The refusals of tld_feat_append.
inline std::string feat_append_check(const void* bank, int64_t capacity, int64_t used, int64_t dim, int64_t pitch, const void* src, int32_t src_dtype,
                                     int64_t rows, int32_t normalize, const void* bad_count) {
    using namespace feat_detail;
    const char* who = "feat append";
    if (!bank) return std::string(who) + ": bank is NULL";
    if (!src) return std::string(who) + ": src is NULL";
    if (!bad_count) return std::string(who) + ": bad_count is NULL";
    const std::string w = check_width(who, dim, pitch);
    if (!w.empty()) return w;
    if (src_dtype < 0 || src_dtype > 2) return std::string(who) + say(": src_dtype %lld (fp32 0, bf16 1, fp16 2)", src_dtype, 0);
    if (normalize != 0 && normalize != 1) return std::string(who) + say(": normalize %lld (0 or 1)", normalize, 0);
    if (rows < 1) return std::string(who) + say(": rows %lld (at least 1)", (long long)rows, 0);
    if (capacity < 1 || used < 0 || used > capacity || rows > capacity - used)
        return std::string(who) + say(": rows [%lld, +%lld)", (long long)used, (long long)rows) + say(" do not fit a bank of %lld rows", (long long)capacity, 0);
    return std::string();
}

// The refusals of tld_feat_moments.
inline std::string feat_moments_check(const void* bank, int64_t n, int64_t dim, int64_t pitch, const void* mean, const void* cov) {
    using namespace feat_detail;
    const char* who = "feat moments";
    if (!bank) return std::string(who) + ": bank is NULL";
    if (!mean) return std::string(who) + ": mean is NULL";
    if (!cov) return std::string(who) + ": cov is NULL";
    const std::string w = check_width(who, dim, pitch);
    if (!w.empty()) return w;
    if (n < 2) return std::string(who) + say(": n %lld (the sample covariance needs at least 2 rows)", (long long)n, 0);
    return std::string();
}

}  // namespace tld

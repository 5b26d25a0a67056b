// tld_opt_plan.h -- the work list of the grouped optimizer step (tld_train.hip: tld_opt_plan_create): a pure function from
// the segment (tensor) lengths of the flat parameter vector to the chunks the kernels take one workgroup each, and the argument checks of
// tld_opt_plan_create.  No HIP in this file: tests/host/opt_plan_main.cpp compiles it on its own and tests/test_opt_groups_host.py restates the cut.
//
// The cut: the segments tile [0, numel) in order; segment s of n elements becomes ceil(n / OPT_CHUNK) chunks, each OPT_CHUNK long but the last,
// laid from the segment's first element.  No chunk spans two segments, so a chunk has ONE group and its partial sum belongs to ONE tensor.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace tld {

constexpr int64_t OPT_CHUNK = 8192;                        // elements per chunk at most: FIXED (not a function of the CU count), a multiple of 4
constexpr int64_t OPT_MAX_NUMEL = (int64_t)1 << 40;
constexpr int32_t OPT_MAX_GROUPS = 256;
static_assert(OPT_CHUNK % 4 == 0, "16-byte accesses on aligned interiors");

struct OptChunk { int64_t first; int32_t len; int32_t seg; };          // elements [first, first + len) of segment seg

struct OptGroup { float lr_scale; float weight_decay; int32_t frozen; int32_t reserved; };      // = tld_opt_group (include/tld_hip.h)

struct OptCut {
    int64_t numel = 0;
    std::vector<OptChunk> chunks;
    std::vector<int64_t> seg_chunk0;                       // [n_seg + 1]: segment s owns chunks [seg_chunk0[s], seg_chunk0[s + 1])
};

inline int64_t opt_chunks_of(int64_t n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

// chunks of the whole list without building them (0 when a length is < 1)
inline int64_t opt_chunk_count(const int64_t* seg_numel, int32_t n_seg) {
    int64_t c = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
        if (seg_numel[s] < 1) return 0;
        c += opt_chunks_of(seg_numel[s]);
    }
    return c;
}

// The cut itself.  The lengths were checked (opt_plan_check): every one >= 1, the total <= OPT_MAX_NUMEL.
inline OptCut opt_cut(const int64_t* seg_numel, int32_t n_seg) {
    OptCut cut;
    cut.chunks.reserve((size_t)opt_chunk_count(seg_numel, n_seg));
    cut.seg_chunk0.reserve((size_t)n_seg + 1);
    int64_t pos = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
        cut.seg_chunk0.push_back((int64_t)cut.chunks.size());
        const int64_t n = seg_numel[s];
        for (int64_t o = 0; o < n; o += OPT_CHUNK) cut.chunks.push_back(OptChunk{pos + o, (int32_t)(n - o < OPT_CHUNK ? n - o : OPT_CHUNK), s});
        pos += n;
    }
    cut.seg_chunk0.push_back((int64_t)cut.chunks.size());
    cut.numel = pos;
    return cut;
}

// The refusals of tld_opt_plan_create, in the order of include/tld_hip.h; "" when the arguments are good.  Every text names the offending index.
inline std::string opt_plan_check(const int64_t* seg_numel, const int32_t* seg_group, int32_t n_seg, const OptGroup* groups, int32_t n_groups,
                                  const float* lr_factors, int64_t n_factors, const void* out) {
    char b[160];
    auto say = [&b](const char* fmt, long long i, double v) { std::snprintf(b, sizeof b, fmt, i, v); return std::string(b); };
    if (!seg_numel) return "seg_numel is NULL";
    if (!seg_group) return "seg_group is NULL";
    if (!groups) return "groups is NULL";
    if (!out) return "out is NULL";
    if (n_seg < 1) return say("n_seg %lld (at least one segment)", n_seg, 0.0);
    if (n_groups < 1 || n_groups > OPT_MAX_GROUPS) return say("n_groups %lld outside [1, 256]", n_groups, 0.0);
    if (n_factors < 0) return say("n_factors %lld", (long long)n_factors, 0.0);
    if (n_factors > 0 && !lr_factors) return say("lr_factors is NULL with n_factors %lld", (long long)n_factors, 0.0);
    for (int32_t q = 0; q < n_groups; ++q) {
        const OptGroup& g = groups[q];
        if (!std::isfinite(g.lr_scale) || g.lr_scale < 0.0f) return say("group %lld: lr_scale %g (finite and >= 0)", q, g.lr_scale);
        if (!std::isfinite(g.weight_decay) || g.weight_decay < 0.0f) return say("group %lld: weight_decay %g (finite and >= 0)", q, g.weight_decay);
        if (g.frozen != 0 && g.frozen != 1) return say("group %lld: frozen %g (0 or 1)", q, (double)g.frozen);
    }
    for (int64_t j = 0; j < n_factors; ++j)
        if (!std::isfinite(lr_factors[j]) || lr_factors[j] < 0.0f) return say("lr factor %lld: %g (finite and >= 0)", (long long)j, lr_factors[j]);
    int64_t total = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
        if (seg_numel[s] < 1) return say("segment %lld: length %g (at least 1)", s, (double)seg_numel[s]);
        if (seg_group[s] < 0 || seg_group[s] >= n_groups) return say("segment %lld: group %g out of range", s, (double)seg_group[s]);
        if (seg_numel[s] > OPT_MAX_NUMEL - total) return say("segment %lld: the total length passes 2^40 (%g)", s, (double)total + (double)seg_numel[s]);
        total += seg_numel[s];
    }
    return std::string();
}

}  // namespace tld

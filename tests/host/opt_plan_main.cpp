// Stand-alone check of csrc/tld_opt_plan.h (the cut of the grouped optimizer step's work list and the argument checks of tld_opt_plan_create),
// built by tests/test_opt_groups_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     opt_plan_main CASES.txt        one segment list per line: "name n0 n1 n2 ..."
//
// For every list it checks that the chunks tile [0, numel) in order, that none is empty, longer than OPT_CHUNK or spans two segments, that a chunk
// shorter than OPT_CHUNK is the last of its segment, and that the per-segment chunk ranges are exact; then it prints
//     name numel n_chunks chunk_digest range_digest
// (digests mod 2^64: tests/opt_groups_ref.py restates them).  A broken property prints the case and makes the exit status 1.  The lists are handled
// as arithmetic only: nothing is allocated per element.
#include "tld_opt_plan.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <sstream>

using namespace tld;

static int check_cut(const std::string& name, const std::vector<int64_t>& seg) {
    const int32_t n_seg = (int32_t)seg.size();
    const OptCut cut = opt_cut(seg.data(), n_seg);
    auto bad = [&name](const char* what, long long at) { std::printf("%s: BROKEN %s at %lld\n", name.c_str(), what, at); return 1; };
    if ((int64_t)cut.chunks.size() != opt_chunk_count(seg.data(), n_seg)) return bad("chunk count", (long long)cut.chunks.size());
    if ((int32_t)cut.seg_chunk0.size() != n_seg + 1 || cut.seg_chunk0[0] != 0 || cut.seg_chunk0[(size_t)n_seg] != (int64_t)cut.chunks.size())
        return bad("range table ends", n_seg);
    int64_t pos = 0, c = 0;
    for (int32_t s = 0; s < n_seg; ++s) {
        if (cut.seg_chunk0[(size_t)s] != c) return bad("range start", s);
        const int64_t seg_end = pos + seg[(size_t)s];
        while (pos < seg_end) {
            if (c >= (int64_t)cut.chunks.size()) return bad("ran out of chunks", s);
            const OptChunk& k = cut.chunks[(size_t)c];
            if (k.first != pos) return bad("tiling", c);
            if (k.seg != s) return bad("segment of chunk", c);
            if (k.len < 1 || k.len > OPT_CHUNK) return bad("chunk length", c);
            if (k.first + k.len > seg_end) return bad("chunk spans two segments", c);
            if (k.len < OPT_CHUNK && k.first + k.len != seg_end) return bad("short chunk inside a segment", c);
            pos += k.len; ++c;
        }
        if (cut.seg_chunk0[(size_t)s + 1] != c) return bad("range end", s);
    }
    if (c != (int64_t)cut.chunks.size() || pos != cut.numel) return bad("total", c);
    uint64_t dc = 0, dr = 0;
    for (size_t i = 0; i < cut.chunks.size(); ++i) {
        const OptChunk& k = cut.chunks[i];
        dc += (((uint64_t)k.first * 1000003u + (uint64_t)k.len) * 31u + (uint64_t)k.seg) * (uint64_t)(i + 1);
    }
    for (int32_t s = 0; s < n_seg; ++s) dr += (uint64_t)cut.seg_chunk0[(size_t)s] * (uint64_t)(s + 1);
    dr += (uint64_t)cut.seg_chunk0[(size_t)n_seg];
    std::printf("%s %" PRId64 " %zu %" PRIu64 " %" PRIu64 "\n", name.c_str(), cut.numel, cut.chunks.size(), dc, dr);
    return 0;
}

// the refusals, each by the index it must name
static int check_refusals() {
    const int64_t numel[3] = {5, 1, 9};
    const int32_t group[3] = {0, 1, 0};
    const OptGroup groups[2] = {{1.0f, 0.0f, 0, 0}, {0.5f, 0.1f, 1, 0}};
    const float factors[2] = {0.5f, 1.0f};
    void* out = nullptr;
    int fails = 0;
    auto expect = [&fails](const std::string& got, const char* want) {
        if (got.find(want) == std::string::npos) { std::printf("refusal: wanted '%s', got '%s'\n", want, got.c_str()); ++fails; }
    };
    expect(opt_plan_check(numel, group, 3, groups, 2, factors, 2, &out), "");
    if (!opt_plan_check(numel, group, 3, groups, 2, factors, 2, &out).empty()) ++fails;
    expect(opt_plan_check(nullptr, group, 3, groups, 2, factors, 2, &out), "seg_numel is NULL");
    expect(opt_plan_check(numel, group, 0, groups, 2, factors, 2, &out), "n_seg 0");
    const int64_t zero_len[3] = {5, 0, 9};
    expect(opt_plan_check(zero_len, group, 3, groups, 2, factors, 2, &out), "segment 1: length");
    const int32_t bad_group[3] = {0, 1, 2};
    expect(opt_plan_check(numel, bad_group, 3, groups, 2, factors, 2, &out), "segment 2: group");
    OptGroup g2[2] = {groups[0], groups[1]};
    g2[1].weight_decay = std::numeric_limits<float>::quiet_NaN();
    expect(opt_plan_check(numel, group, 3, g2, 2, factors, 2, &out), "group 1: weight_decay");
    g2[1] = groups[1]; g2[0].frozen = 2;
    expect(opt_plan_check(numel, group, 3, g2, 2, factors, 2, &out), "group 0: frozen");
    const float neg[2] = {0.5f, -1.0f};
    expect(opt_plan_check(numel, group, 3, groups, 2, neg, 2, &out), "lr factor 1");
    expect(opt_plan_check(numel, group, 3, groups, 2, nullptr, 2, &out), "lr_factors is NULL");
    const int64_t huge[3] = {OPT_MAX_NUMEL - 1, 1, 1};
    expect(opt_plan_check(huge, group, 3, groups, 2, factors, 2, &out), "segment 2: the total length passes 2^40");
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
        std::string name;
        if (!(ls >> name)) continue;
        std::vector<int64_t> seg;
        for (int64_t n; ls >> n;) seg.push_back(n);
        const std::vector<int32_t> group(seg.size(), 0);
        const OptGroup neutral{1.0f, 0.0f, 0, 0};
        if (!opt_plan_check(seg.data(), group.data(), (int32_t)seg.size(), &neutral, 1, nullptr, 0, &fails).empty()) {
            std::printf("%s: REFUSED\n", name.c_str());
            ++fails;
            continue;
        }
        fails += check_cut(name, seg);
    }
    std::printf("chunk %" PRId64 " %d failures\n", OPT_CHUNK, fails);
    return fails ? 1 : 0;
}

// Stand-alone driver of csrc/tld_launch_plan.h (the launches of the inference forward's row and attention kernels: DESIGN.md section 7.22), built by
// tests/test_launch_plan_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     launch_plan_main CASES.txt
//
// One launch per line, whitespace-separated; one line of integers comes back: form gx gy gz block groups lds paths, then the site's own fields
//     embed batch ntok pd cpp d held                 tpw nj half
//     ln    M d mx8                                  nq nj half
//     cross batch ntok d heads x_in f8 cus           nq gpw nj cps half mode_outputs
//     skf   M d                                      cpl
//     tail  batch ntok pd d hid held cus             nt rt nj rows_per_block half
//     dw    batch grid channels f8                   f8, and whether tld_debug_dwconv_gelu refuses the size (tld_reach.h)
//     attn  batch ntok heads                         kt nw nbuf npairs, and whether tld_debug_attention_fwd refuses the size
#include "tld_reach.h"

#include <fstream>
#include <iostream>
#include <sstream>

using namespace tld;

static void geom(const LaunchGeom& g, int form) {
    std::printf("%d %u %u %u %u %lld %d %llu", form, g.gx, g.gy, g.gz, g.block, (long long)g.groups, g.lds, (unsigned long long)g.paths);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        int a[7] = {0};
        const int n = what == "embed" ? 6 : what == "ln" ? 3 : what == "cross" ? 7 : what == "skf" ? 2 : what == "tail" ? 7 : what == "dw" ? 4 : what == "attn" ? 3 : -1;
        if (n < 0) { std::fprintf(stderr, "unknown query %s\n", what.c_str()); return 2; }
        for (int k = 0; k < n; ++k) in >> a[k];
        if (!in) { std::fprintf(stderr, "%s: a short line\n", what.c_str()); return 2; }
        if (what == "embed") {
            const EmbedPlan p = plan_embed(a[0], a[1], a[2], a[3], a[4], a[5] != 0);
            geom(p, p.form); std::printf(" %d %d %d\n", p.tpw, p.nj, (int)p.half);
        } else if (what == "ln") {
            const LayerNormPlan p = plan_layernorm(a[0], a[1], a[2] != 0);
            geom(p, p.form); std::printf(" %d %d %d\n", p.nq, p.nj, (int)p.half);
        } else if (what == "cross") {
            const CrossRowPlan p = plan_cross_row(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0, a[6]);
            geom(p, p.form); std::printf(" %d %d %d %d %d %d\n", p.nq, p.gpw, p.nj, p.cps, (int)p.half, (int)p.mode_outputs);
        } else if (what == "skf") {
            const SplitkFinishPlan p = plan_splitk_finish(a[0], a[1]);
            geom(p, p.form); std::printf(" %d\n", p.cpl);
        } else if (what == "tail") {
            const TailPlan p = plan_tail(a[0], a[1], a[2], a[3], a[4] != 0, a[5] != 0, a[6]);
            geom(p, p.form); std::printf(" %d %d %d %d %d\n", p.nt, p.rt, p.nj, p.rows_per_block, (int)p.half);
        } else if (what == "dw") {
            const DwconvPlan p = plan_dwconv(a[0], a[1], a[2], a[3] != 0);
            geom(p, p.form); std::printf(" %d %d\n", (int)p.f8, (int)!dwconv_hook_refusal(a[0], a[1], a[2]).empty());
        } else {
            const AttentionPlan p = plan_attention(a[0], a[1], a[2]);
            geom(p, p.form); std::printf(" %d %d %d %lld %d\n", p.kt, p.nw, p.nbuf, (long long)p.npairs, (int)!attention_fwd_hook_refusal(a[0], a[1], a[2]).empty());
        }
    }
    return 0;
}

// Stand-alone driver of csrc/tld_reach.h (the sizes the kernels' 32-bit offsets and 16-bit grid axes end at, as refusals: DESIGN.md section 7.19), built by
// tests/test_large_offsets_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     reach_main CASES.txt
//
// One query per line, whitespace-separated; one JSON object per line comes back, {"refusal": "..."} ("" where the size is accepted):
//     train  image_size noise_embed_dims patch_size embed_dim n_layers text_emb_size n_channels mlp_multiplier max_batch      tld_train_create's arithmetic
//            + "gemms": launches of the step checked against launch_gemm's reach, "unfit": how many of them it would refuse, "untested": weight-gradient
//              splits the step's plan chooses that are not among them (accepted configurations only)
//     clip   max_batch rows width patch_rows patch_k            tld_clip_create (patch_rows 0) / tld_clip_vis_create
//     dwconv batch grid channels                                tld_debug_dwconv_gelu
//     attn_fwd batch ntok heads | attn_bwd batch ntok heads     tld_debug_attention_fwd / _bwd
//     wgrad  rows n_out k_in                                    tld_debug_wgrad
//     gemm   M N K lda ldw f8 w_batch_rows w_batch_stride_bytes tld_debug_gemm_epilogue (launch_gemm's own check)
#include "tld_reach.h"

#include <fstream>
#include <iostream>
#include <sstream>
#include <vector>

using namespace tld;

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
}

static bool fits(const TrainGemm& g) {
    GemmParams p{};
    p.M = (int)g.M; p.N = (int)g.N; p.K = (int)g.K; p.lda = (int)g.lda; p.ldw = (int)g.ldw; p.w_batch_rows = (int)g.w_batch_rows; p.w_batch_stride_bytes = (unsigned)g.w_batch_stride_bytes;
    return g.M <= 2147483647L && g.w_batch_stride_bytes < (1ull << 32) && gemm_offsets_fit(p) != 0;
}

// Every launch_gemm call a training step of max_batch samples can make (train_gemms, csrc/tld_train_plan.h: the linears, and the transposing weight gradient at
// EVERY split count its workspace admits) against launch_gemm's reach; and that the split the step's plan chooses -- at 256 and at 304 CUs, with
// TLD_TRAIN_TN_WGRAD=0 -- is one of the shapes just tested.
static void train_gemm_reach(const tld_config& c, long* total, long* unfit, long* untested) {
    const TrainShape s = train_shape(c);
    const TrainWorkspace w = train_workspace(s);
    const std::vector<TrainGemm> all = train_gemms(s, w, c.max_batch);
    for (const TrainGemm& g : all) { ++*total; if (!fits(g)) ++*unfit; }
    const int shape[4][2] = {{s.d, s.hid}, {s.hid, s.d}, {s.d, s.d}, {3 * s.d, s.d}};      // (Nout, Kin) of plan.wg[]
    for (int cus : {256, 304}) {
        const TrainStepPlan p = train_step_plan(s, w, c.max_batch, cus, false);
        for (int k = 0; k < 4; ++k) {
            bool found = false;
            for (const TrainGemm& g : all)
                found = found || (g.sk == p.wg[k].sk && g.M == (long)g.sk * shape[k][0] && g.N == shape[k][1] && g.K == p.wg[k].run_rows);
            if (!found) ++*untested;
        }
    }
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
        std::string r, extra;
        if (what == "train") {
            tld_config c{};
            in >> c.image_size >> c.noise_embed_dims >> c.patch_size >> c.embed_dim >> c.n_layers >> c.text_emb_size >> c.n_channels >> c.mlp_multiplier >> c.max_batch;
            r = train_config_check(c);
            if (r.empty()) {
                long total = 0, unfit = 0, untested = 0;
                train_gemm_reach(c, &total, &unfit, &untested);
                extra = ", \"gemms\": " + std::to_string(total) + ", \"unfit\": " + std::to_string(unfit) + ", \"untested\": " + std::to_string(untested);
            }
        } else if (what == "clip") {
            int mb, rows, width, pr, pk;
            in >> mb >> rows >> width >> pr >> pk;
            r = clip_reach_check(mb, rows, width, pr, pk);
        } else if (what == "dwconv" || what == "attn_fwd" || what == "attn_bwd" || what == "wgrad") {
            int a, b, c3;
            in >> a >> b >> c3;
            r = what == "dwconv" ? dwconv_hook_refusal(a, b, c3) : what == "attn_fwd" ? attention_fwd_hook_refusal(a, b, c3)
                : what == "attn_bwd" ? attention_bwd_hook_refusal(a, b, c3) : wgrad_hook_refusal(a, b, c3);
        } else if (what == "gemm") {
            GemmParams p{};
            in >> p.M >> p.N >> p.K >> p.lda >> p.ldw >> p.f8 >> p.w_batch_rows >> p.w_batch_stride_bytes;
            r = gemm_hook_refusal(p);
        } else { std::fprintf(stderr, "unknown query %s\n", what.c_str()); return 2; }
        if (!in) { std::fprintf(stderr, "%s: a short line\n", what.c_str()); return 2; }
        std::printf("{\"refusal\": %s%s}\n", quoted(r).c_str(), extra.c_str());
    }
    return 0;
}

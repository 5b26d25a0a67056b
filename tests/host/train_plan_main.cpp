// Stand-alone driver of csrc/tld_train_plan.h (the host decisions of the training step: shape, workspace, weight-gradient split, attention-backward dispatch,
// the plan of a step and its predicted launch-path mask), built by tests/test_train_plan_host.py with the host compiler alone, once plain
// and once with -fsanitize=address,undefined.
//
//     train_plan_main CASES.txt
//
// One query per line, whitespace-separated; one JSON object per line comes back:
//     plan  image_size noise_embed_dims patch_size embed_dim n_layers text_emb_size n_channels mlp_multiplier max_batch   batch cus tn_wgrad
//           the refusal of tld_train_create's arithmetic; if there is none the shape, the workspace, every field of the plan of a step of `batch` samples, what each
//           site asks of the partial-sum buffer [site, floats], and "fits": the largest of those demands over EVERY batch 1 .. max_batch, which must not exceed
//           part_floats
//     wgrad M Nout Kin cus slice_floats tr_rows      one weight-gradient product: [form, sk, run_rows] with TLD_TRAIN_TN_WGRAD on ("tn") and off ("tr")
//     attn  ntok has_stats                           the attention backward's dispatch
#include "tld_reach.h"

#include <fstream>
#include <iostream>
#include <sstream>

using namespace tld;

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
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
        if (what == "plan") {
            tld_config c{};
            int batch = 0, cus = 0, tn = 0;
            in >> c.image_size >> c.noise_embed_dims >> c.patch_size >> c.embed_dim >> c.n_layers >> c.text_emb_size >> c.n_channels >> c.mlp_multiplier >> c.max_batch >> batch >>
                cus >> tn;
            if (!in) { std::fprintf(stderr, "plan: a short line\n"); return 2; }
            const std::string bad = train_config_check(c);
            std::printf("{\"refusal\": %s", quoted(bad).c_str());
            if (!bad.empty()) { std::printf("}\n"); continue; }
            const TrainShape s = train_shape(c);
            const TrainWorkspace w = train_workspace(s);
            const TrainStepPlan p = train_step_plan(s, w, batch, cus, tn != 0);
            std::printf(", \"shape\": {\"d\": %d, \"L\": %d, \"H\": %d, \"G\": %d, \"N\": %d, \"pd\": %d, \"hid\": %d, \"S\": %d, \"C\": %d, \"ne\": %d, \"text\": %d, \"max_batch\": %d}", s.d, s.L,
                        s.H, s.G, s.N, s.pd, s.hid, s.S, s.C, s.ne, s.text, s.max_batch);
            std::printf(", \"workspace\": {\"part_floats\": %zu, \"splitk_floats\": %zu, \"tr_rows\": %zu, \"zero_bias\": %zu, \"attn_stats\": %zu, \"scr\": %zu}", w.part_floats,
                        w.splitk_floats, w.tr_rows, w.zero_bias, w.attn_stats, w.scr);
            std::printf(", \"plan\": {\"batch\": %d, \"M\": %d, \"embed_lds\": %d, \"embed_wgs\": %d, \"resid_q4\": %d, \"lnb_q4\": %d, \"tail4\": %d, \"dw_fused\": %d, \"dw_rows\": %d, "
                        "\"dw_grid\": %d, \"dw_lds\": %zu, \"dw_bwd_grid\": %d, \"dw_bwd_lds\": %zu, \"attn\": [%d, %d, %d], \"paths\": %llu", p.batch, p.M, p.embed_lds, p.embed_wgs,
                        p.resid_q4, p.lnb_q4, p.tail4, (int)p.dw_fused, p.dw_rows, p.dw_grid, p.dw_lds, p.dw_bwd_grid, p.dw_bwd_lds, p.attn.mode, p.attn.waves, (int)p.attn.masked,
                        (unsigned long long)p.paths);
            std::printf(", \"tall\": [");
            for (int k = 0; k < 3; ++k) std::printf("%s[%d, %d, %zu]", k ? ", " : "", p.tall[k].nn, p.tall[k].K, p.tall[k].demand);
            std::printf("], \"colsum\": [");
            for (int k = 0; k < 3; ++k) std::printf("%s[%d, %d, %d, %zu]", k ? ", " : "", (int)p.colsum[k].used, (int)p.colsum[k].four, p.colsum[k].cols, p.colsum[k].demand);
            std::printf("], \"wg\": [");
            for (int k = 0; k < 4; ++k) std::printf("%s[%d, %d, %d]", k ? ", " : "", p.wg[k].form, p.wg[k].sk, p.wg[k].run_rows);
            std::printf("]}, \"demands\": [");
            PartDemand dm[10];
            const int nd = train_part_demands(p, dm);
            for (int k = 0; k < nd; ++k) std::printf("%s[%s, %zu]", k ? ", " : "", quoted(dm[k].site).c_str(), dm[k].floats);
            size_t worst = 0; int worst_batch = 0;      // every batch the engine accepts
            for (int b = 1; b <= c.max_batch; ++b) {
                const TrainStepPlan q = train_step_plan(s, w, b, cus, tn != 0);
                const int n = train_part_demands(q, dm);
                for (int k = 0; k < n; ++k) if (dm[k].floats > worst) { worst = dm[k].floats; worst_batch = b; }
            }
            std::printf("], \"fits\": {\"largest_demand\": %zu, \"at_batch\": %d}}\n", worst, worst_batch);
        } else if (what == "wgrad") {
            int M, Nout, Kin, cus;
            TrainWorkspace w{};
            in >> M >> Nout >> Kin >> cus >> w.splitk_floats >> w.tr_rows;
            if (!in) { std::fprintf(stderr, "wgrad: a short line\n"); return 2; }
            const WgradPlan a = wgrad_plan(M, Nout, Kin, cus, true, w), b = wgrad_plan(M, Nout, Kin, cus, false, w);
            std::printf("{\"tn\": [%d, %d, %d], \"tr\": [%d, %d, %d]}\n", a.form, a.sk, a.run_rows, b.form, b.sk, b.run_rows);
        } else if (what == "attn") {
            int ntok, has_stats;
            in >> ntok >> has_stats;
            if (!in) { std::fprintf(stderr, "attn: a short line\n"); return 2; }
            const AttnBwdDispatch a = attn_bwd_dispatch(ntok, has_stats != 0);
            std::printf("{\"mode\": %d, \"waves\": %d, \"masked\": %d, \"path\": %d}\n", a.mode, a.waves, (int)a.masked, a.path());
        } else { std::fprintf(stderr, "unknown query %s\n", what.c_str()); return 2; }
    }
    return 0;
}

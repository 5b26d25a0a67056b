// Stand-alone driver of csrc/tld_body_plan.h (the mode of an inference engine: refusals, switches, plan, held images, reserved stages), built by
// tests/test_body_plan_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     body_plan_main CASES.txt
//
// CASES.txt holds one engine per line, whitespace-separated:
//     name image_size noise_embed_dims patch_size embed_dim n_layers text_emb_size n_channels mlp_multiplier max_batch device_id   ndev cus   ops   NAME=value ...
// ndev: the device count tld_engine_create sees.  ops: what is called on the engine after create, a comma-separated list of d0 | d1 (tld_engine_set_gemm_dtype),
// c<N> (tld_engine_set_low_latency) and F (tld_engine_finalize_weights), or "-" for none.  NAME=value: the environment at create.
// The driver goes through the calls as the engine does -- a refused setter changes nothing -- and prints one JSON object per line: the refusal of create; if there
// is none the refusal of every op ("" where it passed), the shape, the switches after the ops, every field of the plan, every row of the image table
// [member, stage name, dtype, numel, margin, held], every reserved stage [name, bytes], and every GEMM launch of a forward of max_batch samples against
// launch_gemm's own reach check [name, fits with bf16 operands, fits with fp8 operands]; and "launch", what the plan meets in csrc/tld_launch_plan.h: the form of the
// quantising LayerNorm where ln_mx8 is set, whether cross_row has the outputs fold_ln3 / cross_mx8 ask for, the form of the split-K finish where ll_split is set (-1
// each where the plan does not ask), and the launch-path bits of the row and attention launches of a forward of max_batch samples, plain and with a shared layer 0.
#include "tld_body_plan.h"

#include <fstream>
#include <iostream>
#include <map>
#include <sstream>

using namespace tld;

static std::string quoted(const std::string& s) {
    std::string o = "\"";
    for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; }
    return o + "\"";
}

// The row and attention launches run_body (csrc/tld_engine.hip) makes under a plan, each site's `paths` or-ed together.  shared: the CFG-doubled batch with layer-0
// sharing -- embed, LayerNorm-1 and attention of block 0 on half the samples, block 0's cross_row fanning out.  (The split-bf16 images outside the blocks are always held.)
static uint64_t forward_paths(const BodyShape& s, const BodyPlan& P, int batch, bool shared) {
    const int b0 = shared ? batch / 2 : batch;
    uint64_t m = plan_embed(b0, s.ntok, s.pd, s.pd, s.d, true).paths;
    for (int l = 0; l < s.L; ++l) {
        const bool half = shared && l == 0;
        const int bl = half ? b0 : batch;
        if (!P.fold_ln1) m |= plan_layernorm(bl * s.ntok, s.d, P.ln_mx8).paths;
        if (!P.fused_qa) m |= plan_attention(bl, s.ntok, s.H).paths;
        m |= plan_cross_row(batch, s.ntok, s.d, s.H, half, P.cross_mx8, P.cus).paths;
        if (!P.fuse_dw) m |= plan_dwconv(batch, s.grid, s.hid, P.dw_mx8).paths;
        if (P.ll_split && !(l + 1 == s.L && P.fold_tail)) m |= plan_splitk_finish(batch * s.ntok, s.d).paths;
    }
    return m | plan_tail(batch, s.ntok, s.pd, s.d, P.fold_tail, true, P.cus).paths;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASES.txt\n", argv[0]); return 2; }
    std::ifstream file(argv[1]);
    if (!file) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(file, line)) {
        std::istringstream in(line);
        std::string name, ops;
        if (!(in >> name)) continue;
        tld_config c{};
        int ndev = 0, cus = 0;
        in >> c.image_size >> c.noise_embed_dims >> c.patch_size >> c.embed_dim >> c.n_layers >> c.text_emb_size >> c.n_channels >> c.mlp_multiplier >> c.max_batch >>
            c.device_id >> ndev >> cus >> ops;
        if (!in) { std::fprintf(stderr, "%s: a short line\n", name.c_str()); return 2; }
        std::map<std::string, std::string> env;
        for (std::string kv; in >> kv;) env[kv.substr(0, kv.find('='))] = kv.substr(kv.find('=') + 1);

        std::printf("{\"name\": %s", quoted(name).c_str());
        std::string bad = body_config_check(c, -1);          // (tld_engine_create: the device count is asked for after the refusals in front of the device_id one)
        if (bad.empty()) bad = body_config_check(c, ndev);
        std::printf(", \"create\": %s", quoted(bad).c_str());
        if (!bad.empty()) { std::printf("}\n"); continue; }

        const BodyShape s = body_shape(c);
        BodySwitches sw = body_switches([&env](const char* k) -> const char* { auto it = env.find(k); return it == env.end() ? nullptr : it->second.c_str(); });
        BodyPlan plan = plan_body(s, sw, false, 0, c.max_batch, cus);
        bool finalized = false;
        int splitk_slices = 0;
        std::printf(", \"ops\": [");
        std::istringstream opl(ops == "-" ? "" : ops);
        bool first = true;
        for (std::string op; std::getline(opl, op, ',');) {
            std::string r;
            const int v = op.size() > 1 ? std::atoi(op.c_str() + 1) : 0;
            if (op == "F") finalized = true;
            else if (op[0] == 'c') {
                r = body_class_refusal(s, c.max_batch, v, plan.fp8);
                if (r.empty()) {
                    if (lowlat_split(v)) splitk_slices = lowlat_split(v);
                    plan = plan_body(s, sw, plan.fp8, v, c.max_batch, cus, finalized ? &plan : nullptr);
                }
            } else if (op[0] == 'd') {
                r = finalized ? "(state) the GEMM operand type must be chosen before tld_engine_finalize_weights" : body_dtype_refusal(s, v, plan.cls);
                if (r.empty()) { body_switches_set_dtype(sw, v); plan = plan_body(s, sw, v == 1, plan.cls, c.max_batch, cus); }
            } else { std::fprintf(stderr, "%s: unknown op %s\n", name.c_str(), op.c_str()); return 2; }
            std::printf("%s%s", first ? "" : ", ", quoted(r).c_str());
            first = false;
        }
        std::printf("], \"shape\": {\"d\": %d, \"L\": %d, \"H\": %d, \"grid\": %d, \"ntok\": %d, \"pd\": %d, \"hid\": %d, \"img\": %d, \"ne\": %d, \"text\": %d}", s.d, s.L, s.H, s.grid,
                    s.ntok, s.pd, s.hid, s.img, s.ne, s.text);
        std::printf(", \"switches\": {\"fold_ln1\": %d, \"fold_ln3\": %d, \"fold_tail\": %d, \"fuse_dwconv\": %d, \"fuse_qkv_attn\": %d, \"fp8_fused\": %d, \"qkv_pair\": %d, "
                    "\"share_l0\": %d, \"guidance_skip\": %d}", sw.fold_ln1, sw.fold_ln3, sw.fold_tail, sw.fuse_dwconv, sw.fuse_qkv_attn, sw.fp8_fused, sw.qkv_pair, sw.share_l0,
                    sw.guidance_skip);
        const BodyPlan& p = plan;
        std::printf(", \"plan\": {\"fp8\": %d, \"cls\": %d, \"heads\": %d, \"cus\": %d, \"share_l0\": %d, \"guidance_skip\": %d, \"fold_ln1\": %d, \"fold_ln3\": %d, \"fused_qa\": %d, "
                    "\"pair_held\": %d, \"pair\": %d, \"pair_always\": %d, \"pair_slots\": %lld, \"fuse_dw\": %d, \"seam\": %d, \"fold_tail_held\": %d, \"fold_tail\": %d, \"ln_mx8\": %d, "
                    "\"cross_mx8\": %d, \"dw_mx8\": %d, \"quant_qkv\": %d, \"quant_up\": %d, \"quant_down\": %d, \"ll_split\": %d}", p.fp8, p.cls, p.heads, p.cus, p.share_l0,
                    p.guidance_skip, p.fold_ln1, p.fold_ln3, p.fused_qa, p.pair_held, p.pair, p.pair_always, (long long)p.pair_slots, p.fuse_dw, p.seam, p.fold_tail_held, p.fold_tail,
                    p.ln_mx8, p.cross_mx8, p.dw_mx8, p.quant_qkv, p.quant_up, p.quant_down, p.ll_split);
        std::printf(", \"pair_launch\": \"");      // which launches of 1 .. max_batch samples take two-head tiles: one character each
        for (int b = 1; b <= c.max_batch; ++b) std::printf("%d", (int)body_pair_launch(p, b));
        std::printf("\", \"images\": [");
        Layer ly;                                  // the table's offsets, used as finalize uses them: every held member is set, and none twice
        int k = 0;
        for (const BodyImage& q : body_block_images(s, p)) {
            if (q.get(ly)) { std::fprintf(stderr, "%s: two rows for member %s\n", name.c_str(), q.id); return 3; }
            q.set(ly, &ly);
            std::printf("%s[%s, %s, %d, %lld, %lld, %d]", k++ ? ", " : "", quoted(q.id).c_str(), quoted(q.name ? q.name : "").c_str(), q.dtype, (long long)q.numel(),
                        (long long)q.margin, q.held);
        }
        std::printf("], \"stages\": [");
        k = 0;
        for (const BodyStage& st : body_stages(s, p, c.max_batch, splitk_slices)) std::printf("%s[%s, %zu]", k++ ? ", " : "", quoted(st.name).c_str(), st.bytes);
        // every launch_gemm call of a forward of max_batch samples against the launch's own reach check, bf16 and fp8 operands: [name, fits, fits in fp8 mode]
        std::printf("], \"gemm_reach\": [");
        BodyGemm gb[3], g8[3];
        const int ng = body_gemms(c, s.grid, c.max_batch, false, gb);
        body_gemms(c, s.grid, c.max_batch, true, g8);
        for (k = 0; k < ng; ++k) std::printf("%s[%s, %d, %d]", k ? ", " : "", quoted(gb[k].name).c_str(), (int)body_gemm_fits(gb[k]), (int)body_gemm_fits(g8[k]));
        std::printf("], \"launch\": [%d, %d, %d, %llu, %llu]}\n", p.ln_mx8 ? (int)plan_layernorm(c.max_batch * s.ntok, s.d, true).form : -1,
                    p.fold_ln3 || p.cross_mx8 ? (int)plan_cross_row(c.max_batch, s.ntok, s.d, s.H, false, p.cross_mx8, cus).mode_outputs : -1,
                    p.ll_split ? (int)plan_splitk_finish(c.max_batch * s.ntok, s.d).form : -1, (unsigned long long)forward_paths(s, p, c.max_batch, false),
                    (unsigned long long)forward_paths(s, p, c.max_batch, true));
    }
    return 0;
}

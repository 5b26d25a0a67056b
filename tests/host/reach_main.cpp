// Stand-alone driver of csrc/tld_reach.h (the sizes the kernels' 32-bit offsets and 16-bit grid axes end at, as refusals: DESIGN.md section 7.19), built by
// tests/test_large_offsets_host.py with the host compiler alone, once plain and once with -fsanitize=address,undefined.
//
//     reach_main CASES.txt
//
// One query per line, whitespace-separated; one JSON object per line comes back, {"refusal": "..."} ("" where the size is accepted):
//     train  image_size noise_embed_dims patch_size embed_dim n_layers text_emb_size n_channels mlp_multiplier max_batch      tld_train_create's arithmetic
//            + "gemms": launches of the step checked against launch_gemm's reach, "unfit": how many of them it would refuse (accepted configurations only)
//     clip   max_batch rows width patch_rows patch_k            tld_clip_create (patch_rows 0) / tld_clip_vis_create
//     dwconv batch grid channels                                tld_debug_dwconv_gelu
//     attn_fwd batch ntok heads | attn_bwd batch ntok heads     tld_debug_attention_fwd / _bwd
//     wgrad  rows n_out k_in                                    tld_debug_wgrad
//     gemm   M N K lda ldw f8 w_batch_rows w_batch_stride_bytes tld_debug_gemm_epilogue (launch_gemm's own check)
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

static bool fits(long M, long N, long K, long lda, long ldw, long wbr = 0, unsigned long long wbs = 0) {
    GemmParams p{};
    p.M = (int)M; p.N = (int)N; p.K = (int)K; p.lda = (int)lda; p.ldw = (int)ldw; p.w_batch_rows = (int)wbr; p.w_batch_stride_bytes = (unsigned)wbs;
    return M <= 2147483647L && wbs < (1ull << 32) && gemm_offsets_fit(p) != 0;
}

// Every launch_gemm call a training step of max_batch samples can make, by shape: the linears of the forward and of the input gradients (A = an activation of M
// rows), and the transposing weight gradient dW[Nout, Kin] = dY^T X for EVERY split count its workspace admits (tld_train.hip: weight_grad -- the step picks
// one of them by the CU count; all are checked here): A = T1 [sk Nout, ms], W = T2 with the block-diagonal offset of split sk - 1.
static void train_gemms(const tld_config& c, long* total, long* unfit) {
    const long G = c.image_size / c.patch_size, M = (long)c.max_batch * G * G, d = c.embed_dim, hid = d * c.mlp_multiplier;
    const long tr_rows = M + kTrainTransposeMargin;
    auto count = [&](bool ok) { ++*total; if (!ok) ++*unfit; };
    const long widths[4] = {d, 2 * d, 3 * d, hid};
    for (long k : widths) for (long n : widths) count(fits(M, n, k, k, k));
    const long pairs[5][2] = {{d, hid}, {hid, d}, {3 * d, d}, {d, d}, {2 * d, d}};
    for (const auto& pr : pairs) {
        const long Nout = pr[0], Kin = pr[1];
        const long ms1 = (M + 63) / 64 * 64;
        count(fits(Nout, Kin, ms1, ms1, ms1));
        for (long sk = 2; sk <= 32; ++sk) {
            const long mp = ((M + sk - 1) / sk + 127) / 128 * 128;
            if (sk * mp > tr_rows) continue;
            count(fits(sk * Nout, Kin, mp, mp, mp, Nout, (unsigned long long)Kin * mp * 2));
        }
        for (long sk = 2; sk <= 8; sk *= 2) if (M % sk == 0) count(fits(sk * Nout, Kin, M / sk, M / sk, M / sk, Nout, (unsigned long long)Kin * (M / sk) * 2));
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
                long total = 0, unfit = 0;
                train_gemms(c, &total, &unfit);
                extra = ", \"gemms\": " + std::to_string(total) + ", \"unfit\": " + std::to_string(unfit);
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

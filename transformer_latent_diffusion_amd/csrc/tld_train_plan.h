// tld_train_plan.h -- the host decisions of the training step (tld_train.hip, tld_train_attn.hip): the derived shape of a configuration,
// every workspace capacity that is not "rows x width of one activation", the split of a weight-gradient product, the dispatch of the attention backward, and the
// plan of one step of `batch` samples -- the form and the size-dependent launch geometry at every dispatch site, what each site asks of the partial-sum buffer,
// and the mask of launch-path bits the step will set.  A pure function of (configuration, batch, CU count, TLD_TRAIN_TN_WGRAD).  No HIP in this file:
// tests/host/train_plan_main.cpp compiles it on its own and tests/test_train_plan_host.py holds it against the restatement in tests/train_plan_ref.py.
// Every rule is written ONCE here; the engine makes a plan per batch size and its launch sites switch on the fields.  The sites keep their own PATH(...) calls
// inside the branch that launches, so the mask tld_train_debug_paths reports is evidence independent of the one predicted here.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/tld_hip.h"

namespace tld {

// launch-path bits (the table in include/tld_hip.h)
enum : int {
    PB_RESID_Q4 = 0, PB_RESID_GEN = 4, PB_LNB_Q4 = 5, PB_LNB_GEN = 8, PB_EMB_LDS = 9, PB_EMB_PLAIN = 13, PB_TAIL4_16 = 14, PB_TAIL4_32 = 15, PB_TAIL4_64 = 16,
    PB_TAIL_GEN = 17, PB_TALL_COLS = 18, PB_TALL_PART = 19, PB_COLSUM4 = 20, PB_COLSUM = 21, PB_DW_FUSED = 22, PB_DW_UNFUSED = 23, PB_WG_TN = 24,
    PB_WG_TR1 = 25, PB_WG_TRSK = 26, PB_WG_PAD = 27, PB_ATT_ONE = 28, PB_ATT_TWO = 29, PB_ATT_MASKED = 30
};
static_assert(PB_ATT_MASKED + 1 == TLD_TRAIN_PATH_BITS, "the table of include/tld_hip.h");

constexpr int kTrainTransposeMargin = 4096;       // rows T1 / T2 hold beyond M: split-K runs padded to a multiple of 128 rows

// ---- the depthwise kernels (tld_train_kernels.h) ------------------------------------------------------------------------------------------------------------
// dwconv_kernel works on bands of image rows, one halo row on each side, [rows][G tokens][64 channels] bf16 in LDS
inline int dwconv_band_rows(int G) { return G < 16 ? G : 16; }
inline size_t dwconv_lds_bytes(int G) { const int R = dwconv_band_rows(G); return (size_t)(R + 2 < G ? R + 2 : G) * G * 128; }
// the fused backward holds both images of a (sample, 64-channel chunk) in LDS
inline bool train_dw_fused(int G, int N, int hid) { return G <= 16 && N >= 176 && hid % 64 == 0; }

// ---- the derived shape of a configuration (after train_config_check, tld_reach.h) ----------------------------------------------------------------------------
struct TrainShape { int d, L, H, G, N, pd, hid, S, C, ne, text, max_batch; };
inline TrainShape train_shape(const tld_config& c) {
    TrainShape s{};
    s.d = c.embed_dim; s.L = c.n_layers; s.H = s.d / 64; s.G = c.image_size / c.patch_size; s.N = s.G * s.G; s.S = c.image_size; s.C = c.n_channels;
    s.pd = s.C * c.patch_size * c.patch_size; s.hid = s.d * c.mlp_multiplier; s.ne = c.noise_embed_dims; s.text = c.text_emb_size; s.max_batch = c.max_batch;
    return s;
}

inline size_t chunks_of(size_t rows, size_t per) { return (rows + per - 1) / per; }

// ---- who writes partial sums to the engine's `part` buffer, and how many floats for `rows` rows ----------------------------------------------------------------
inline size_t ln_bwd_part(size_t rows, size_t width) { return chunks_of(rows, 32) * 2 * width; }         // (dgamma | dbeta) per 32-row workgroup
inline size_t ln_small_part(size_t rows, size_t pd) { return chunks_of(rows, 256) * 2 * pd; }           // the patch LayerNorm: per 256-row workgroup
inline bool colsum_by_four(size_t rows, size_t cols) { return cols % 4 == 0 && rows >= 4096; }          // four columns per thread, 64-row chunks (the chunk count feeds the 64 part-lanes of the reduction)
inline size_t colsum_part(size_t rows, size_t cols) { return chunks_of(rows, colsum_by_four(rows, cols) ? 64 : 256) * cols; }
inline bool tall_dw_has_cols(int Nn) { return Nn == 16 || Nn == 32 || Nn == 64; }                      // tall_dw_cols_partial<TX, Nn> exists
inline size_t tall_dw_cols_part(size_t rows, size_t Nn, size_t K) { return chunks_of(rows, 64) * Nn * K; }
inline size_t tall_dw_rows_part(size_t rows, size_t Nn, size_t K) { return chunks_of(rows, 256) * Nn * K; }
inline size_t dw_bwd_part(bool fused, size_t batch, size_t G, size_t hid) { return fused ? batch * 11 * hid : batch * G * 10 * hid; }   // per sample [11][hid] / per (sample, image row) [10][hid]

// ---- the workspace: every capacity tld_train_create allocates that is not rows x width of one activation --------------------------------------------------------
struct TrainWorkspace {
    size_t part_floats;       // reduction partials: the largest demand of any site at max_batch
    size_t splitk_floats;     // split-K slices of the weight gradients [8][max(hid, 3 d)][d]
    size_t tr_rows;           // rows of the transposed split-K operands T1 / T2 (each tr_rows x max(hid, 3 d) bf16)
    size_t zero_bias;         // floats of the all-zero bias vector
    size_t attn_stats;        // attention backward above 256 tokens: [B, H, 2, N] (log-sum-exp | delta)
    size_t scr;               // small fp32 scratch ([pd, d], + 64)
};
inline TrainWorkspace train_workspace(const TrainShape& s) {
    const size_t B = (size_t)s.max_batch, M = B * s.N, d = (size_t)s.d, hid = (size_t)s.hid, pd = (size_t)s.pd, wide = hid > 3 * d ? hid : 3 * d;
    TrainWorkspace w{};
    w.zero_bias = 3 * hid > 4096 ? 3 * hid : 4096;
    w.attn_stats = 2 * M * s.H;
    w.scr = pd * d + 64;
    w.tr_rows = M + kTrainTransposeMargin;
    w.splitk_floats = 8 * wide * d;
    size_t need = chunks_of(M, 256) * 2 * wide;                                        // LayerNorm / column-sum partials of 256-row chunks
    auto atleast = [&need](size_t n) { if (n > need) need = n; };
    atleast(ln_bwd_part(M, d));                                                        // LayerNorm-backward partials (32-row workgroups)
    atleast(dw_bwd_part(false, B, (size_t)s.G, hid));                                  // depthwise weight-gradient partials (per sample and image row)
    atleast(chunks_of(M, 64) * wide);                                                  // column-sum partials (64-row chunks)
    atleast(tall_dw_cols_part(M, pd, d));                                              // tall weight-gradient partials (64-row chunks)
    w.part_floats = need;
    return w;
}

// ---- the split of a weight-gradient product dW[Nout, Kin] = dY^T X over M rows -----------------------------------------------------------------------------------
// The output is small and the contraction long, so the rows are cut into `sk` runs of run_rows rows (split-K into fp32 slices [sk][Nout][Kin], summed in a fixed
// order: bit-reproducible).  With 256 x 256 tiles a launch has sk (Nout / 256) (Kin / 256) workgroups: the chooser takes the count whose last round of tiles is
// fullest (e.g. 7 x 12 x 3 = 252 of 256 CUs for the up-projection weight), discounted by the zero padding of the runs.  ONE loop serves both forms; what differs
// between them is the rule:
struct WgradRule {
    int align;          // runs are padded to a multiple of this many rows
    int first;          // the first candidate count
    int min_rows;       // fewer rows than this: no scoring
    bool bounded_rows;  // sk run_rows must fit the transposed operands (tr_rows)
};
constexpr WgradRule kWgradUntransposed{64, 1, 0, false};      // launch_gemm_tn reads dY and X as they are: any 64-row run, one run allowed, no operand copies to fit
constexpr WgradRule kWgradTransposing{128, 2, 4096, true};    // T1 / T2 hold [sk][width][run_rows]
struct WgradSplit { int sk, run_rows; };

inline int wgrad_run_rows(long M, int c, int align) { return (int)(((M + c - 1) / c + align - 1) / align * align); }
// the rows of c runs fit the transposed operands: THE workspace rule of the transposing form (tests/host/reach_main.cpp walks every count it admits)
inline bool wgrad_rows_fit(int c, long run_rows, size_t tr_rows) { return (size_t)c * (size_t)run_rows <= tr_rows; }
// Where nothing is scored: the power-of-two split of the first transposing form -- halve while the halves stay multiples of 128 rows and at least 1024 long, at
// most 8 runs.  It decides wherever the scored loop does not run (fewer than 4096 rows; a width that is no multiple of 256, e.g. d = 128 or 192 with hid = 4 d)
// and only there: with 4096 rows or more two runs are always admissible.  The first such shape: M = 2048, TLD_TRAIN_TN_WGRAD=0, d = 256 (sk 2, runs of 1024).
// M is a multiple of 16 (train_config_check), so a halving that passes leaves no remainder, and M % 64 != 0 gives sk = 1.
inline WgradSplit wgrad_pow2_split(int M, int Nout) {
    int sk = 1;
    if (Nout % 256 == 0) while (sk < 8 && (M / (sk * 2)) % 128 == 0 && M / (sk * 2) >= 1024) sk *= 2;
    return WgradSplit{sk, M / sk};
}
inline WgradSplit wgrad_split(int M, int Nout, int Kin, int cus, const WgradRule& r, size_t slice_floats, size_t tr_rows) {
    WgradSplit best = wgrad_pow2_split(M, Nout);
    if (Nout % 256 || Kin % 256 || M % 64 || M < r.min_rows) return best;
    const long per = (long)(Nout / 256) * (Kin / 256);
    double top = 0.0;
    for (int c = r.first; c <= 32; ++c) {
        const int mp = wgrad_run_rows(M, c, r.align);
        if ((c > 1 && mp < 1024) || (long)(c - 1) * mp >= M) continue;                                      // runs too short / last run empty
        if (c > 1 && (size_t)c * Nout * Kin > slice_floats) continue;                                       // slice workspace
        if (r.bounded_rows && !wgrad_rows_fit(c, mp, tr_rows)) continue;                                     // operand workspace
        const long tiles = per * c, rounds = (tiles + cus - 1) / cus;
        const double eff = (double)tiles / (double)(rounds * cus) * ((double)M / ((double)c * mp));
        if (eff > top + 1e-9) { top = eff; best = WgradSplit{c, mp}; }
    }
    return best;
}

// what launch_gemm_tn takes
inline bool wgrad_untransposed_takes(int M, int Nout, int Kin) { return Nout % 256 == 0 && Kin % 256 == 0 && M % 64 == 0 && M > 0; }

enum WgradForm : int { WG_TN = PB_WG_TN, WG_TR1 = PB_WG_TR1, WG_TRSK = PB_WG_TRSK, WG_PAD = PB_WG_PAD };      // (each form is its path bit)
struct WgradPlan { int form, sk, run_rows; };
// One product of the step.  WG_TN: both operands as they are.  Else both transposed so that the contraction is contiguous: one run (WG_TR1), stacked runs and one
// batched GEMM (WG_TRSK), or -- M no multiple of 64, e.g. 144 x 3 rows -- one run zero-padded to the next multiple of 64, the GEMM's K step (WG_PAD).
inline WgradPlan wgrad_plan(int M, int Nout, int Kin, int cus, bool tn_wgrad, const TrainWorkspace& w) {
    if (tn_wgrad && wgrad_untransposed_takes(M, Nout, Kin)) {
        const WgradSplit s = wgrad_split(M, Nout, Kin, cus, kWgradUntransposed, w.splitk_floats, 0);
        return WgradPlan{WG_TN, s.sk, s.run_rows};
    }
    if (M % 64) return WgradPlan{WG_PAD, 1, (M + 63) / 64 * 64};
    const WgradSplit s = wgrad_split(M, Nout, Kin, cus, kWgradTransposing, w.splitk_floats, w.tr_rows);
    return WgradPlan{s.sk == 1 ? WG_TR1 : WG_TRSK, s.sk, s.run_rows};
}

// ---- the attention backward (tld_train_attn.hip) -----------------------------------------------------------------------------------------------------------------
// Waves per workgroup (block width BT = 32 nw tokens) at N tokens (N a multiple of 16).  N <= 256: one block holds the sample, nw = ceil(N / 32) (64 / 128 / 256
// tokens: 2 / 4 / 8, exact).  N > 256: the nw in 4 .. 8 with the least padded length ceil(N / BT) BT, the wider on a tie (a multiple of 256: 8); 7 only where it
// leaves no padding -- the masked 7-wave dQ kernel spills.  Padded work (Np / N)^2 at the square grids: 16 tokens 4.0 (one 32-token tile), 144: 1.23, 400: 1.44,
// 784: 1.04, 1296: 1.08, 1936: 1.12, 2704: 1.01, 3600: 1.03; 576, 1600, 3136 and the multiples of 256 none.
inline int attn_bwd_block_waves(int ntok) {
    if (ntok <= 256) return (ntok + 31) / 32;
    int best = 8, pad = 1 << 30;
    for (int nw = 8; nw >= 4; --nw) {
        const int bt = 32 * nw, np = (ntok + bt - 1) / bt * bt;
        if (nw == 7 && np != ntok) continue;
        if (np < pad) { pad = np; best = nw; }
    }
    return best;
}
enum AttnBwdMode : int { ATTN_BWD_REFUSED = 0, ATTN_BWD_ONE = 1, ATTN_BWD_TWO = 2 };      // (the values of launch_attention_bwd's path_out, | 4 masked)
struct AttnBwdDispatch {
    int mode;          // one kernel per (sample, head), or the dQ kernel + the dK / dV kernel with the row statistics between them
    int waves;         // attn_bwd_kernel<waves, ...>
    bool masked;       // the token count is no multiple of the block: the MASKED instantiation
    int path() const { return mode | (masked ? 4 : 0); }
};
// has_stats: the caller gave the statistics scratch the two-kernel form needs.  Refused: a token count that is no positive multiple of 16, or above 256 without scratch.
inline AttnBwdDispatch attn_bwd_dispatch(int ntok, bool has_stats) {
    if (ntok <= 0 || ntok % 16 || (ntok > 256 && !has_stats)) return AttnBwdDispatch{ATTN_BWD_REFUSED, 0, false};
    const int nw = attn_bwd_block_waves(ntok);
    return AttnBwdDispatch{ntok <= 256 ? ATTN_BWD_ONE : ATTN_BWD_TWO, nw, ntok % (32 * nw) != 0};
}

// ---- the plan of one step ----------------------------------------------------------------------------------------------------------------------------------------
struct TallDwPlan { int nn; int K; size_t demand; };                     // nn: 16 / 32 / 64 = tall_dw_cols_partial<TX, nn> over 64-row chunks; 0 = tall_dw_partial over 256-row chunks
struct ColsumPlan { bool used; bool four; int cols; size_t demand; };    // four: colsum4_partial over 64-row chunks; else colsum_partial over 256-row chunks
enum { TALL_OUT = 0, TALL_LIN = 1, TALL_CONV = 2 };                      // dWout [pd, d]; the embedding's linear [pd, d]; its convolution [pd, pd]
enum { CS_PD = 0, CS_D = 1, CS_HID = 2 };                                // column sums of M rows by width: out_proj / conv bias; down / linear bias; up bias (unfused depthwise backward only)
enum { WGP_DOWN = 0, WGP_UP = 1, WGP_Q = 2, WGP_QKV = 3 };
struct TrainStepPlan {
    int batch = 0, M = 0;
    int embed_lds = 0;            // embed_fwd_lds_kernel<k> (the [pd, d] weight in LDS: at most 64 KiB), k 256-feature blocks; 0: embed_fwd_kernel
    int embed_wgs = 0;            // its workgroups: four rows each, the LDS form at most four per CU (grid-stride)
    int resid_q4 = 0;             // resid_add_ln_q4_kernel<k> at d = 256 k; 0: the generic pair
    int lnb_q4 = 0;               // ln_bwd_q4_kernel<.., k> at d = 256 k, k <= 3; 0: ln_bwd_kernel
    int tail4 = 0;                // tail_dx4_kernel<pd> at pd 16 / 32 / 64; 0: tail_dx_kernel
    TallDwPlan tall[3];
    ColsumPlan colsum[3];
    bool dw_fused = false;        // GELU' multiply, depthwise weight-gradient partials and input gradient in one pass
    int dw_rows = 0, dw_grid = 0; size_t dw_lds = 0;      // dwconv_kernel (the forward, and the unfused backward's input gradient): band rows, workgroups, LDS bytes
    int dw_bwd_grid = 0; size_t dw_bwd_lds = 0;            // the fused backward: one workgroup per (sample, 64-channel chunk); 0 when unfused
    WgradPlan wg[4];
    AttnBwdDispatch attn{};
    size_t lnb_demand = 0, lnb_cond_demand = 0, ln_small_demand = 0, dw_demand = 0;      // floats of `part`: ln_bwd over M rows, over the 2 B conditioning rows, ...
    uint64_t paths = 0;           // the mask a debug step will report
};
struct PartDemand { const char* site; size_t floats; };
inline int train_part_demands(const TrainStepPlan& p, PartDemand out[10]) {
    int n = 0;
    out[n++] = {"ln_bwd", p.lnb_demand}; out[n++] = {"ln_bwd cond", p.lnb_cond_demand}; out[n++] = {"ln_small_bwd", p.ln_small_demand};
    out[n++] = {"depthwise backward", p.dw_demand};
    const char* tn[3] = {"tall_dw out_proj", "tall_dw linear", "tall_dw conv"};
    for (int k = 0; k < 3; ++k) out[n++] = {tn[k], p.tall[k].demand};
    const char* cn[3] = {"colsum pd", "colsum d", "colsum hid"};
    for (int k = 0; k < 3; ++k) if (p.colsum[k].used) out[n++] = {cn[k], p.colsum[k].demand};
    return n;
}

inline TrainStepPlan train_step_plan(const TrainShape& s, const TrainWorkspace& w, int batch, int cus, bool tn_wgrad) {
    TrainStepPlan p;
    const int d = s.d, hid = s.hid, pd = s.pd, M = batch * s.N;
    auto bit = [&p](int b) { p.paths |= 1ull << b; };
    p.batch = batch; p.M = M;
    const int rows4 = (M + 3) / 4;
    if ((size_t)pd * d * 4 <= 65536) { p.embed_lds = d <= 256 ? 1 : d <= 512 ? 2 : d <= 768 ? 3 : 4; p.embed_wgs = rows4 < 4 * cus ? rows4 : 4 * cus; bit(PB_EMB_LDS + p.embed_lds - 1); }
    else { p.embed_wgs = rows4; bit(PB_EMB_PLAIN); }
    p.resid_q4 = d % 256 == 0 ? d / 256 : 0;                       // (d <= 1024)
    bit(p.resid_q4 ? PB_RESID_Q4 + p.resid_q4 - 1 : PB_RESID_GEN);
    p.lnb_q4 = d % 256 == 0 && d <= 768 ? d / 256 : 0;
    bit(p.lnb_q4 ? PB_LNB_Q4 + p.lnb_q4 - 1 : PB_LNB_GEN);
    p.lnb_demand = ln_bwd_part((size_t)M, (size_t)d); p.lnb_cond_demand = ln_bwd_part(2 * (size_t)batch, (size_t)d); p.ln_small_demand = ln_small_part((size_t)M, (size_t)pd);
    p.tail4 = pd == 16 || pd == 32 || pd == 64 ? pd : 0;
    bit(p.tail4 == 16 ? PB_TAIL4_16 : p.tail4 == 32 ? PB_TAIL4_32 : p.tail4 == 64 ? PB_TAIL4_64 : PB_TAIL_GEN);
    const int tall_k[3] = {d, d, pd};
    for (int k = 0; k < 3; ++k) {      // the column form where it exists and its partials fit (they do at every accepted configuration: tests/test_train_plan_host.py)
        const bool cols = tall_dw_has_cols(pd) && tall_dw_cols_part((size_t)M, (size_t)pd, (size_t)tall_k[k]) <= w.part_floats;
        p.tall[k] = TallDwPlan{cols ? pd : 0, tall_k[k], cols ? tall_dw_cols_part((size_t)M, (size_t)pd, (size_t)tall_k[k]) : tall_dw_rows_part((size_t)M, (size_t)pd, (size_t)tall_k[k])};
        bit(cols ? PB_TALL_COLS : PB_TALL_PART);
    }
    p.dw_fused = train_dw_fused(s.G, s.N, hid);
    bit(p.dw_fused ? PB_DW_FUSED : PB_DW_UNFUSED);
    p.dw_rows = dwconv_band_rows(s.G); p.dw_grid = batch * (hid / 64) * ((s.G + p.dw_rows - 1) / p.dw_rows); p.dw_lds = dwconv_lds_bytes(s.G);
    if (p.dw_fused) { p.dw_bwd_grid = batch * (hid / 64); p.dw_bwd_lds = (size_t)2 * s.N * 128; }
    p.dw_demand = dw_bwd_part(p.dw_fused, (size_t)batch, (size_t)s.G, (size_t)hid);
    const int cs_cols[3] = {pd, d, hid};
    for (int k = 0; k < 3; ++k) {
        const bool used = k != CS_HID || !p.dw_fused;      // (the fused depthwise backward sums the up-projection's bias gradient itself)
        p.colsum[k] = ColsumPlan{used, colsum_by_four((size_t)M, (size_t)cs_cols[k]), cs_cols[k], colsum_part((size_t)M, (size_t)cs_cols[k])};
        if (used) bit(p.colsum[k].four ? PB_COLSUM4 : PB_COLSUM);
    }
    const int wg_shape[4][2] = {{d, hid}, {hid, d}, {d, d}, {3 * d, d}};      // (Nout, Kin): down, up, cross-attention q, qkv
    for (int k = 0; k < 4; ++k) { p.wg[k] = wgrad_plan(M, wg_shape[k][0], wg_shape[k][1], cus, tn_wgrad, w); bit(p.wg[k].form); }
    p.attn = attn_bwd_dispatch(s.N, true);
    if (p.attn.mode == ATTN_BWD_ONE) bit(PB_ATT_ONE);
    if (p.attn.mode == ATTN_BWD_TWO) bit(PB_ATT_TWO);
    if (p.attn.masked) bit(PB_ATT_MASKED);
    return p;
}

// ---- every launch_gemm shape a step of `batch` samples can make ---------------------------------------------------------------------------------------------------
// The linears of the forward and of the input gradients (A = an activation of M rows, every pair of the step's widths), and the transposing weight gradient
// dW[Nout, Kin] = dY^T X at EVERY split its operand workspace admits -- the step picks one of them by the CU count (wgrad_split); all are listed: A = T1
// [sk Nout, run_rows], W = T2 with the block-diagonal offset of split sk - 1.  What tests/host/reach_main.cpp asserts gemm_offsets_fit for at the largest accepted
// max_batch.  sk: 0 a linear; else the split count of a weight-gradient product (K = its run_rows).
struct TrainGemm { long M, N, K, lda, ldw, w_batch_rows; unsigned long long w_batch_stride_bytes; int sk; };
inline std::vector<TrainGemm> train_gemms(const TrainShape& s, const TrainWorkspace& w, int batch) {
    const long M = (long)batch * s.N, d = s.d, hid = s.hid;
    std::vector<TrainGemm> v;
    const long widths[4] = {d, 2 * d, 3 * d, hid};
    for (long k : widths) for (long n : widths) v.push_back(TrainGemm{M, n, k, k, k, 0, 0, 0});
    const long pairs[5][2] = {{d, hid}, {hid, d}, {3 * d, d}, {d, d}, {2 * d, d}};
    auto split = [&v](long Nout, long Kin, int sk, long ms) { v.push_back(TrainGemm{sk * Nout, Kin, ms, ms, ms, sk > 1 ? Nout : 0, sk > 1 ? (unsigned long long)Kin * ms * 2 : 0, sk}); };
    for (const auto& pr : pairs) {
        split(pr[0], pr[1], 1, (M + 63) / 64 * 64);
        for (int sk = kWgradTransposing.first; sk <= 32; ++sk) {
            const long mp = wgrad_run_rows(M, sk, kWgradTransposing.align);
            if (wgrad_rows_fit(sk, mp, w.tr_rows)) split(pr[0], pr[1], sk, mp);
        }
        for (int sk = 2; sk <= 8; sk *= 2) if (M % sk == 0) split(pr[0], pr[1], sk, M / sk);      // the power-of-two runs (wgrad_pow2_split), unpadded
    }
    return v;
}

}  // namespace tld

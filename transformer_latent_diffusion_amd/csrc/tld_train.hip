// tld_train.hip -- the training step of the denoiser on gfx950: C ABI tld_train_*.
//
// Replaces, for one optimisation step of tld/train.py:162-173,
//     pred = model(x_noisy, noise_level.view(-1, 1), label); loss = MSELoss(pred, x); loss.backward()      -> tld_train_forward_backward
//     optimizer.step() (torch.optim.Adam) + update_ema(ema_model, model, alpha)  (tld/train.py:55-58)       -> tld_train_adam_ema
// The gradient all-reduce of accelerate's DDP wrapper stays with the caller (torch.distributed over RCCL on the flat gradient buffer,
// transformer_latent_diffusion_amd/train.py): parameters, gradients, Adam moments and the EMA copy are FLAT fp32 device buffers
// owned by the caller in the canonical order of Denoiser.named_parameters() (tld_train_param_layout).
//
// Arithmetic: fp32 master parameters; the big projections (QKV, cross-attention Q, MLP up / down) and their dX / dW products are
// bf16-operand, fp32-accumulate MFMA GEMMs (tld_gemm.hip); activations that are saved for the backward are bf16; LayerNorm, softmax,
// GELU, the conditioning path, the patch embedding, reductions and the optimizer are fp32.  The training forward is the plain module
// graph (none of the inference path's algebraic folds), so every saved tensor is the one autograd would save.
#include "../../include/tld_hip.h"
#include "tld_train_kernels.h"
#include "tld_host.h"
#include "tld_param_layout.h"
#include "tld_opt_plan.h"
#include "tld_reach.h"          // train_config_check, the hooks' refusals; tld_train_plan.h: the plan every dispatch below follows

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

using namespace tld;
using namespace tld::train;

namespace tld {
// path_out (may be null): which kernels were launched -- 1 one kernel, 2 two kernels, | 4 the masked forms
int launch_attention_bwd(const bf16* qk, const bf16* vt, const bf16* o, const float* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s, int* path_out = nullptr);
int launch_attention_bwd(const bf16* qk, const bf16* vt, const bf16* o, const bf16* g, bf16* dqkv, float* stats, int batch, int ntok, int heads, hipStream_t s, int* path_out = nullptr);
}

namespace {

using Tensor = ParamTensor;      // the flat parameter / gradient vectors: tld_param_layout.h
using LayerP = LayerOffsets;
struct LayerB {          // engine-owned per-layer buffers
    bf16 *wqkv, *wqkv_t, *wq, *wq_t, *wup, *wup_t, *wdown, *wdown_t;          // bf16 GEMM operands and their transposes
    bf16 *x1, *x2, *x3;                                                      // residual stream at the input of the three sub-blocks
    float2 *st1, *st2, *st3;
    bf16 *a1, *a2, *a3, *qk, *vt, *att, *qc, *cr, *h, *hc, *gl, *o;
    float *kvc, *p0;
    float* dww_t;                                                            // depthwise taps, tap-major [9][hid] (refreshed with the operands)
};

inline dim3 g1(size_t n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

}  // namespace

struct tld_train : TrainShape {        // (the derived shape: tld_train_plan.h)
    tld_config cfg{};
    TrainWorkspace ws{};                 // the capacities create allocated
    int cus = 0;                         // compute units of the engine's device
    TrainStepPlan plan_max, plan_last;   // the plan of a step of max_batch samples, and of the last other batch size (step_plan)
    std::vector<Tensor> layout;
    int64_t nparam = 0;
    // offsets of the non-layer tensors
    int64_t ff1w, ff1b, ff3w, ff3b, cvw, cvb, l1w, l1b, liw, lib, l2w, l2b, pos, outw, outb, nw, nb, lbw, lbb;
    std::vector<LayerP> lp;
    std::vector<LayerB> lb;
    float *params = nullptr, *grads = nullptr;
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;     // size of each entry of allocs (the stage hook poisons them)
    bool debug = false;                  // stage hook (tld_train_set_debug)
    uint64_t paths = 0;                  // launch paths of the last debug call
    StageStore stages;                   // the stage hook (tld_host.h)
    float* angular = nullptr;            // sinusoid buffer (not a parameter; tld/transformer_blocks.py:11-15)
    float* zero_bias = nullptr;
    // conditioning path
    float *sinb, *h1, *g1v, *ycat, *y, *dy, *dycat, *dg1;
    float *kvc_all, *dkv_all, *dy_parts;     // per block, contiguous: (k | v) of the conditioning tokens [L][2B, 2d], its gradient, and each block's share of dL/dy [L][2B, d]
    float2* yst;
    // embedding
    float *p16, *p16n, *e, *patches, *de, *dpn, *dp16;
    float2 *est1, *est2;
    bf16* xfin;
    // tail / loss
    float *dout, *row_loss, *io;
    float* pred_scratch = nullptr;       // tld_train_forward_loss with pred_out NULL: [max_batch, C, S, S]
    int last_batch = 0;                  // batch of the last forward (either entry): what row_loss holds for tld_train_sample_loss
    int captured_batch = 0;              // batch of the last forward enqueued on a capturing stream: a graph replays it out of the engine's sight
    // backward scratch
    float* gx;                           // dL/d(residual stream) fp32 [M, d]
    bf16 *gxb, *T1, *T2, *dbig, *dsmall, *dsmall2;
    float* scr;                          // small fp32 scratch ([pd, d])
    float* attn_stats;                   // attention backward at > 256 tokens: [B, H, 2, N] (log-sum-exp | delta)
    float* splitk;                       // split-K partials of the weight-gradient GEMMs [8][max(hid, 3d)][d]
    float* part;                         // reduction partials
    bool weights_fresh = false;
    bool tn_wgrad = true;                // weight gradients without transposed copies (TLD_TRAIN_TN_WGRAD=0: the transposing form, a test hook)
};

namespace {

template <typename T>
int dalloc(tld_train* e, T** p, size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(T)) != hipSuccess) return fail(TLD_ERR_HIP, "hipMalloc of %zu bytes failed", n * sizeof(T));
    e->allocs.push_back(q);
    e->alloc_bytes.push_back(n * sizeof(T));
    *p = reinterpret_cast<T*>(q);
    return 0;
}
#define DALLOC(ptr, n) do { int _r = dalloc(e, &(ptr), (size_t)(n)); if (_r) return _r; } while (0)

// the plan of a step of `batch` samples: made once per batch size
const TrainStepPlan& step_plan(tld_train* e, int batch) {
    if (batch == e->plan_max.batch) return e->plan_max;
    if (batch != e->plan_last.batch) e->plan_last = train_step_plan(*e, e->ws, batch, e->cus, e->tn_wgrad);
    return e->plan_last;
}

// dW[Nout, Kin] = dY^T X (dY [M, Nout], X [M, Kin], bf16 row-major) with both operands as they are -- the contraction index is the row, the MFMA
// fragments come through the transposing LDS read (launch_gemm_tn): no transposed copies (8 transposes per block were 8.4 % of the step).
// The rows are cut into sp.sk runs of sp.run_rows rows (wgrad_split, tld_train_plan.h: split-K into fp32 slices [sk][Nout][Kin], summed in a fixed order).
// (256 x 384 tiles -- 768-byte W rows with a rotating block swizzle, 240 tiles of 10 splits instead of 252 of 7 -- measured 30.80 vs 30.88 ms per step, with
// 17 spilled registers: not kept.)
void wgrad_tn(const bf16* dY, int Nout, const bf16* X, int Kin, int M, WgradSplit sp, float* dW, float* slices, hipStream_t s) {
    GemmParams g{};
    g.A = dY; g.lda = Nout; g.W = X; g.ldw = Kin; g.M = sp.sk * Nout; g.N = Kin; g.K = sp.run_rows; g.tn_ktotal = M; g.ldc = Kin;
    g.c_f32 = sp.sk == 1 ? dW : slices;
    g.w_batch_rows = sp.sk == 1 ? 0 : Nout;
    launch_gemm_tn(g, s);
    if (sp.sk > 1) hipLaunchKernelGGL(sum_slices, dim3((unsigned)(((size_t)Nout * Kin / 4 + 255) / 256)), dim3(256), 0, s, slices, sp.sk, (size_t)Nout * Kin, dW, (size_t)Nout * Kin / 4);
}

// C[Mr, Nc] = A[Mr, K] . W[Nc, K]^T on the engine's MFMA GEMM
int gemm_f32(const bf16* A, int lda, const bf16* W, int ldw, float* C, int Mr, int Nc, int K, hipStream_t s) {
    GemmParams g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = Mr; g.N = Nc; g.K = K; g.c_f32 = C; g.ldc = Nc;
    return launch_gemm(g, EPI_F32, s);
}
int gemm_bf16(const bf16* A, int lda, const bf16* W, int ldw, const float* bias, bf16* out, int Mr, int Nc, int K, hipStream_t s) {
    GemmParams g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.M = Mr; g.N = Nc; g.K = K; g.out_bf16 = out; g.ldo = Nc; g.bias = bias;
    return launch_gemm(g, EPI_BIAS_BF16, s);
}
// ---- stage hook (StageStore, tld_host.h): this engine's names, sizes and poison step.  The names debug_begin references and the names
// reserve_snapshots reserves are disjoint (forward tensors saved for the backward vs copies of the backward's transient buffers) -----------------
// start of a debug call: poison what the kernels are to write, forget the last call's stages, name the saved forward tensors
int debug_begin(tld_train* e, int B, hipStream_t s) {
    const int d = e->d, hid = e->hid, pd = e->pd, N = e->N, H = e->H, M = B * N;
    e->paths = 0;
    StageStore& S = e->stages;
    S.begin_call();
    auto keep = [&](const void* p) {       // constants and the weight operand copies (refreshed before this point) stay
        if (p == e->angular || p == e->zero_bias) return true;
        for (const LayerB& b : e->lb)
            if (p == b.wqkv || p == b.wqkv_t || p == b.wq || p == b.wq_t || p == b.wup || p == b.wup_t || p == b.wdown || p == b.wdown_t || p == b.dww_t) return true;
        return false;
    };
    for (size_t i = 0; i < e->allocs.size(); ++i)
        if (!keep(e->allocs[i])) HIP_TRY(hipMemsetAsync(e->allocs[i], 0xFF, e->alloc_bytes[i], s));
    HIP_TRY(hipMemsetAsync(e->grads, 0xFF, (size_t)e->nparam * 4, s));
    S.ref("sinb", e->sinb, ST_F32, B, e->ne); S.ref("h1", e->h1, ST_F32, B, d); S.ref("g1v", e->g1v, ST_F32, B, d);
    S.ref("ycat", e->ycat, ST_F32, 2 * B, d); S.ref("y", e->y, ST_F32, 2 * B, d); S.ref("yst", e->yst, ST_F32, 2 * B, 2);
    S.ref("p16", e->p16, ST_F32, M, pd); S.ref("p16n", e->p16n, ST_F32, M, pd); S.ref("est1", e->est1, ST_F32, M, 2);
    S.ref("e", e->e, ST_F32, M, d); S.ref("est2", e->est2, ST_F32, M, 2); S.ref("xfin", e->xfin, ST_BF16, M, d);
    S.ref("dout", e->dout, ST_F32, M, pd); S.ref("row_loss", e->row_loss, ST_F32, M);
    for (int i = 0; i < e->L; ++i) {
        const LayerB& b = e->lb[i];
        const std::string p = "blk" + std::to_string(i) + ".";
        const struct { const char* n; const bf16* q; int w; } acts[] = {{"x1", b.x1, d}, {"a1", b.a1, d}, {"qk", b.qk, 2 * d}, {"att", b.att, d}, {"x2", b.x2, d}, {"a2", b.a2, d},
            {"qc", b.qc, d}, {"cr", b.cr, d}, {"x3", b.x3, d}, {"a3", b.a3, d}, {"h", b.h, hid}, {"hc", b.hc, hid}, {"o", b.o, d}};
        for (const auto& a : acts) S.ref(p + a.n, a.q, ST_BF16, M, a.w);
        S.ref(p + "vt", b.vt, ST_BF16, B, H, 64, N);
        S.ref(p + "st1", b.st1, ST_F32, M, 2); S.ref(p + "st2", b.st2, ST_F32, M, 2); S.ref(p + "st3", b.st3, ST_F32, M, 2);
        S.ref(p + "p0", b.p0, ST_F32, M, H); S.ref(p + "kvc", b.kvc, ST_F32, 2 * B, 2 * d);
        S.ref(p + "wqkv", b.wqkv, ST_BF16, 3 * d, d); S.ref(p + "wqkv_t", b.wqkv_t, ST_BF16, d, 3 * d);
        S.ref(p + "wq", b.wq, ST_BF16, d, d); S.ref(p + "wq_t", b.wq_t, ST_BF16, d, d);
        S.ref(p + "wup", b.wup, ST_BF16, hid, d); S.ref(p + "wup_t", b.wup_t, ST_BF16, d, hid);
        S.ref(p + "wdown", b.wdown, ST_BF16, d, hid); S.ref(p + "wdown_t", b.wdown_t, ST_BF16, hid, d);
    }
    return TLD_OK;
}
// set_debug(1): memory for every snapshot a step of max_batch samples takes (the names of the SNAP calls in tld_train_forward_backward_cb)
int reserve_snapshots(tld_train* e) {
    const size_t M = (size_t)e->max_batch * e->N, d = e->d, hid = e->hid, pd = e->pd, B2 = 2 * (size_t)e->max_batch;
#define RES(name, bytes) do { if (int _r = e->stages.reserve(name, bytes)) return _r; } while (0)
    RES("gx.tail", M * d * 4); RES("gxb.tail", M * d * 2);
    const bool dw_fused = e->plan_max.dw_fused;
    for (int i = 0; i < e->L; ++i) {
        const std::string p = "blk" + std::to_string(i) + ".";
        for (const char* n : {"gl", "dg", "dh"}) RES(p + n, M * hid * 2);
        if (!dw_fused) RES(p + "dhc", M * hid * 2);
        for (const char* n : {"gx.in", "gx.ln3", "gx.ln2", "gx.ln1"}) RES(p + n, M * d * 4);
        for (const char* n : {"da3", "dqc", "da2", "da1"}) RES(p + n, M * d * 2);
        RES(p + "dqkv", M * 3 * d * 2); RES(p + "dkv", B2 * 2 * d * 4);
        if (i > 0) RES(p + "gxb.ln1", M * d * 2);
    }
    RES("dy", B2 * d * 4); RES("dycat", B2 * d * 4); RES("dg1", (size_t)e->max_batch * d * 4); RES("de", M * d * 4); RES("dpn", M * pd * 4); RES("dp16", M * pd * 4);
#undef RES
    return TLD_OK;
}
#define PATH(b) do { if (e->debug) e->paths |= 1ull << (b); } while (0)
#define SNAP(...) do { if (e->debug) { if (int _r = e->stages.copy(__VA_ARGS__)) return _r; } } while (0)

// the bf16 GEMM operands, their transposes and the tap-major depthwise taps of the flat parameter vector `src` (the bound parameters for the training
// step; any other vector for tld_train_forward_loss, which clears weights_fresh afterwards)
int refresh_operands(tld_train* e, const float* src, hipStream_t s) {
    const int d = e->d, hid = e->hid;
    auto both = [&](int64_t off, int R, int Cc, bf16* w, bf16* wt) {       // [R, C] fp32 -> bf16 copy and bf16 transpose [C, R]
        hipLaunchKernelGGL((transpose_to_bf16<float>), dim3((Cc + 31) / 32, (R + 31) / 32), dim3(256), 0, s, src + off, Cc, wt, R, R, Cc, 1, w);
    };
    for (int i = 0; i < e->L; ++i) {
        both(e->lp[i].qkv, 3 * d, d, e->lb[i].wqkv, e->lb[i].wqkv_t);
        both(e->lp[i].q, d, d, e->lb[i].wq, e->lb[i].wq_t);
        both(e->lp[i].up_w, hid, d, e->lb[i].wup, e->lb[i].wup_t);
        both(e->lp[i].down_w, d, hid, e->lb[i].wdown, e->lb[i].wdown_t);
        hipLaunchKernelGGL(dw_tapmajor_kernel, g1((size_t)hid * 9), dim3(256), 0, s, src + e->lp[i].dw_w, e->lb[i].dww_t, hid);
    }
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

// The training forward (the plain module graph of tld/denoiser.py, every tensor the backward needs saved in the engine's buffers) on the flat
// parameter vector P, whose operand copies the caller has refreshed; ends in the per-row squared errors (row_loss) and the scalar loss.  Kernel
// launches only.  Shared by tld_train_forward_backward_cb and tld_train_forward_loss.
int train_forward(tld_train* e, const float* P, const float* x_noisy, const float* noise_level, const float* label, const float* target, int B,
                  float* loss_out, float* pred_out, hipStream_t s) {
    const int d = e->d, hid = e->hid, pd = e->pd, N = e->N, H = e->H, M = B * N, G = e->G;
    const dim3 blk(256);
    const TrainStepPlan& plan = step_plan(e, B);
    {
        static PerDeviceOnce once;
        once.run([&] { hipFuncSetAttribute(reinterpret_cast<const void*>(dwconv_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    }
    const float inv_numel = 1.0f / (float)((size_t)B * e->C * e->S * e->S);
    e->last_batch = B;
    {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess) (void)hipGetLastError();       // (a query that fails says nothing about this call's launches)
        else if (cap != hipStreamCaptureStatusNone) e->captured_batch = B;
    }
    // the small fp32 products on the tiled kernel (see tld_train_kernels.h)
    auto lin_fwd = [&](const float* in, int ldi, const float* W, const float* bias, float* out, int ldo, int R, int Nn, int K, float* pre, int gelu) {
        hipLaunchKernelGGL(tiled_f32_kernel, dim3((Nn + 31) / 32, (R + 31) / 32), dim3(256), 0, s, in, (long)ldi, 1L, W, (long)K, 1L, bias, out, ldo, R, Nn, K, pre, gelu, 0);
    };

    // conditioning (tld/denoiser.py:105-122): sinusoid -> Linear -> GELU -> Linear | label_proj -> stack -> LayerNorm
    hipLaunchKernelGGL(sinusoid_kernel, g1((size_t)B * e->ne / 2), blk, 0, s, noise_level, e->angular, e->sinb, B, e->ne / 2);
    lin_fwd(e->sinb, e->ne, P + e->ff1w, P + e->ff1b, e->g1v, d, B, d, e->ne, e->h1, 1);
    lin_fwd(e->g1v, d, P + e->ff3w, P + e->ff3b, e->ycat, 2 * d, B, d, d, nullptr, 0);
    lin_fwd(label, e->text, P + e->lbw, P + e->lbb, e->ycat + d, 2 * d, B, d, e->text, nullptr, 0);
    hipLaunchKernelGGL((ln_fwd_kernel<float>), dim3((2 * B + 3) / 4), blk, 0, s, e->ycat, P + e->nw, P + e->nb, (bf16*)nullptr, e->y, e->yst,
                       (const float*)nullptr, 1, 2 * B, d);
    // patch embedding (tld/denoiser.py:34-45,75-77)
    {
        EmbedTrain q{};
        q.x = x_noisy; q.conv_w = P + e->cvw; q.conv_b = P + e->cvb; q.ln1_w = P + e->l1w; q.ln1_b = P + e->l1b; q.lin_w = P + e->liw; q.lin_b = P + e->lib;
        q.ln2_w = P + e->l2w; q.ln2_b = P + e->l2b; q.pos = P + e->pos; q.p = e->p16; q.pn = e->p16n; q.st1 = e->est1; q.e = e->e; q.st2 = e->est2;
        q.x0 = e->lb[0].x1; q.B = B; q.C = e->C; q.S = e->S; q.patch = e->cfg.patch_size; q.grid = G; q.pd = pd; q.d = d;
        const size_t lwb = (size_t)pd * d * 4;
        const dim3 grid(plan.embed_wgs);
        switch (plan.embed_lds) {
        case 1: PATH(PB_EMB_LDS); hipLaunchKernelGGL((embed_fwd_lds_kernel<1>), grid, blk, lwb, s, q); break;
        case 2: PATH(PB_EMB_LDS + 1); hipLaunchKernelGGL((embed_fwd_lds_kernel<2>), grid, blk, lwb, s, q); break;
        case 3: PATH(PB_EMB_LDS + 2); hipLaunchKernelGGL((embed_fwd_lds_kernel<3>), grid, blk, lwb, s, q); break;
        case 4: PATH(PB_EMB_LDS + 3); hipLaunchKernelGGL((embed_fwd_lds_kernel<4>), grid, blk, lwb, s, q); break;
        default: PATH(PB_EMB_PLAIN); hipLaunchKernelGGL(embed_fwd_kernel, grid, blk, 0, s, q); break;
        }
    }
    // x_out = x_in + delta [; a_out = LN(x_out), stats]   (delta == nullptr: LayerNorm of x_in alone)
    auto resid_ln = [&](const bf16* x_in, const bf16* delta, bf16* x_out, const float* gamma, const float* beta, bf16* a_out, float2* st) {
        const dim3 grid((M + 3) / 4);
        switch (plan.resid_q4) {
        case 3: PATH(PB_RESID_Q4 + 2); hipLaunchKernelGGL((resid_add_ln_q4_kernel<3>), grid, blk, 0, s, x_in, delta, x_out, gamma, beta, a_out, st, M); break;
        case 2: PATH(PB_RESID_Q4 + 1); hipLaunchKernelGGL((resid_add_ln_q4_kernel<2>), grid, blk, 0, s, x_in, delta, x_out, gamma, beta, a_out, st, M); break;
        case 1: PATH(PB_RESID_Q4); hipLaunchKernelGGL((resid_add_ln_q4_kernel<1>), grid, blk, 0, s, x_in, delta, x_out, gamma, beta, a_out, st, M); break;
        case 4: PATH(PB_RESID_Q4 + 3); hipLaunchKernelGGL((resid_add_ln_q4_kernel<4>), grid, blk, 0, s, x_in, delta, x_out, gamma, beta, a_out, st, M); break;
        default:
            PATH(PB_RESID_GEN);
            if (delta) hipLaunchKernelGGL(resid_add_ln_kernel, grid, blk, 0, s, x_in, delta, x_out, gamma, beta, a_out, st, M, d);
            else hipLaunchKernelGGL((ln_fwd_kernel<bf16>), grid, blk, 0, s, x_in, gamma, beta, a_out, (float*)nullptr, st, (const float*)nullptr, 1, M, d);
            break;
        }
    };
    // (k | v) of the two conditioning tokens for every block in one launch (tld/transformer_blocks.py:66-68): the blocks' parameters are laid out
    // identically, so block i's kv_linear.weight sits i block-strides after block 0's
    const long blk_stride = e->L > 1 ? (long)(e->lp[1].kv - e->lp[0].kv) : 0;
    const long kv_stride = (long)e->max_batch * 2 * 2 * d;
    hipLaunchKernelGGL(tiled_f32_kernel, dim3((2 * d + 31) / 32, (2 * B + 31) / 32, e->L), dim3(256), 0, s, e->y, (long)d, 1L, P + e->lp[0].kv, (long)d, 1L,
                       (const float*)nullptr, e->kvc_all, 2 * d, 2 * B, 2 * d, d, (float*)nullptr, 0, 0, 0L, blk_stride, kv_stride);
    for (int i = 0; i < e->L; ++i) {
        LayerB& b = e->lb[i]; const LayerP& p = e->lp[i];
        // x = x + SA(LN1 x)   (tld/transformer_blocks.py:51-59,136)
        if (i == 0) resid_ln(b.x1, (const bf16*)nullptr, (bf16*)nullptr, P + p.n1w, P + p.n1b, b.a1, b.st1);      // (blocks > 0: LN1 rides on the previous block's last residual add)
        {
            GemmParams g{};
            g.A = b.a1; g.lda = d; g.W = b.wqkv; g.ldw = d; g.M = M; g.N = 3 * d; g.K = d; g.out_bf16 = b.qk; g.ldo = 2 * d; g.vt = b.vt; g.ntok = N; g.d = d;
            GEMM_TRY("training step", launch_gemm(g, EPI_QKV, s));
        }
        launch_attention(b.qk, b.vt, b.att, B, N, H, s);
        resid_ln(b.x1, b.att, b.x2, P + p.n2w, P + p.n2b, b.a2, b.st2);
        // x = x + CA(LN2 x, y)   (:62-72,137)
        GEMM_TRY("training step", gemm_bf16(b.a2, d, b.wq, d, e->zero_bias, b.qc, M, d, d, s));
        hipLaunchKernelGGL(cross_fwd_kernel, dim3(B * H), blk, 0, s, b.qc, b.kvc, b.cr, b.p0, N, d);
        resid_ln(b.x2, b.cr, b.x3, P + p.n3w, P + p.n3b, b.a3, b.st3);
        // x = x + MLPSepConv(LN3 x)   (:89-113,138)
        GEMM_TRY("training step", gemm_bf16(b.a3, d, b.wup, d, P + p.up_b, b.h, M, hid, d, s));
        hipLaunchKernelGGL(dwconv_kernel, dim3(plan.dw_grid), blk, plan.dw_lds, s, b.h, b.dww_t, P + p.dw_b, b.hc, b.gl, B, G, hid, 0, plan.dw_rows);
        GEMM_TRY("training step", gemm_bf16(b.gl, hid, b.wdown, hid, P + p.down_b, b.o, M, d, hid, s));
        bf16* xnext = i + 1 < e->L ? e->lb[i + 1].x1 : e->xfin;
        if (i + 1 < e->L) resid_ln(b.x3, b.o, xnext, P + e->lp[i + 1].n1w, P + e->lp[i + 1].n1b, e->lb[i + 1].a1, e->lb[i + 1].st1);      // + the next block's LN1
        else resid_ln(b.x3, b.o, xnext, (const float*)nullptr, (const float*)nullptr, (bf16*)nullptr, (float2*)nullptr);
    }
    // out_proj + unpatchify + MSE (tld/denoiser.py:47-52,72,82; tld/train.py:167)
    hipLaunchKernelGGL(tail_fwd_kernel, dim3((M + 3) / 4), blk, 0, s, e->xfin, P + e->outw, P + e->outb, target, pred_out, e->dout, e->row_loss, B, e->C, e->S,
                       e->cfg.patch_size, G, pd, d, inv_numel);
    hipLaunchKernelGGL(loss_reduce_kernel, dim3(1), blk, 0, s, e->row_loss, M, inv_numel, loss_out);
    return TLD_OK;
}

}  // namespace

extern "C" {

int tld_train_create(const tld_config* cfg, tld_train** out) {
    if (!cfg || !out) return fail(TLD_ERR_INVALID, "null argument");
    // every refusal that is arithmetic on the configuration, the 32-bit reach of the step's kernels among them (tld_reach.h): before any HIP call
    if (const std::string bad = train_config_check(*cfg); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TLD_ERR_HIP, "no HIP device: the training engine has no CPU path");
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(TLD_ERR_INVALID, "device_id %d out of range", cfg->device_id);
    DeviceGuard dg(cfg->device_id);
    tld_train* e = new tld_train();
    e->cfg = *cfg;
    static_cast<TrainShape&>(*e) = train_shape(*cfg);
    e->ws = train_workspace(*e);
    e->cus = device_cu_count();
    e->tn_wgrad = !(getenv("TLD_TRAIN_TN_WGRAD") && atoi(getenv("TLD_TRAIN_TN_WGRAD")) == 0);
    e->plan_max = train_step_plan(*e, e->ws, e->max_batch, e->cus, e->tn_wgrad);
    const int d = e->d, hid = e->hid, pd = e->pd;
    {   // canonical order: Denoiser.named_parameters() of the reference (tld_param_layout.h; pinned by tests/test_train_host.py)
        const ParamLayout pl = make_param_layout(d, e->L, e->ne, pd, hid, e->N, e->text);
        e->layout = pl.tensors; e->nparam = pl.count; e->lp = pl.layers;
        e->ff1w = pl.ff1w; e->ff1b = pl.ff1b; e->ff3w = pl.ff3w; e->ff3b = pl.ff3b; e->cvw = pl.cvw; e->cvb = pl.cvb; e->l1w = pl.l1w; e->l1b = pl.l1b;
        e->liw = pl.liw; e->lib = pl.lib; e->l2w = pl.l2w; e->l2b = pl.l2b; e->pos = pl.pos; e->outw = pl.outw; e->outb = pl.outb; e->nw = pl.nw; e->nb = pl.nb;
        e->lbw = pl.lbw; e->lbb = pl.lbb;
    }

    const size_t B = e->max_batch, M = B * e->N;      // (M hid 2 < 4 GiB and (M + 4096) max(hid, 3 d) 2 < 4 GiB: train_config_check above)
    auto cleanup = [&](int rc) { for (void* p : e->allocs) hipFree(p); delete e; return rc; };
    auto alloc_all = [&]() -> int {
        DALLOC(e->angular, e->ne / 2); DALLOC(e->zero_bias, e->ws.zero_bias);
        DALLOC(e->sinb, B * e->ne); DALLOC(e->h1, B * d); DALLOC(e->g1v, B * d); DALLOC(e->ycat, B * 2 * d); DALLOC(e->y, B * 2 * d);
        DALLOC(e->dy, B * 2 * d); DALLOC(e->dycat, B * 2 * d); DALLOC(e->dg1, B * d); DALLOC(e->dkv_all, (size_t)e->L * B * 2 * 2 * d); DALLOC(e->kvc_all, (size_t)e->L * B * 2 * 2 * d);
        DALLOC(e->dy_parts, (size_t)e->L * B * 2 * d); DALLOC(e->yst, B * 2);
        DALLOC(e->p16, M * pd); DALLOC(e->p16n, M * pd); DALLOC(e->e, M * d); DALLOC(e->patches, M * pd); DALLOC(e->de, M * d);
        DALLOC(e->dpn, M * pd); DALLOC(e->dp16, M * pd); DALLOC(e->est1, M); DALLOC(e->est2, M); DALLOC(e->xfin, M * d);
        DALLOC(e->dout, M * pd); DALLOC(e->row_loss, M); DALLOC(e->io, 4); DALLOC(e->pred_scratch, B * e->C * e->S * e->S);
        const size_t wide = hid > 3 * d ? hid : 3 * d;
        DALLOC(e->gx, M * d); DALLOC(e->gxb, M * d); DALLOC(e->T1, e->ws.tr_rows * wide); DALLOC(e->T2, e->ws.tr_rows * wide); DALLOC(e->dbig, M * hid);
        DALLOC(e->dsmall, M * 3 * d); DALLOC(e->dsmall2, M * d); DALLOC(e->attn_stats, e->ws.attn_stats); DALLOC(e->scr, e->ws.scr);
        DALLOC(e->splitk, e->ws.splitk_floats);
        DALLOC(e->part, e->ws.part_floats);
        e->lb.resize(e->L);
        for (int i = 0; i < e->L; ++i) {
            LayerB& q = e->lb[i];
            DALLOC(q.wqkv, 3 * d * d); DALLOC(q.wqkv_t, 3 * d * d); DALLOC(q.wq, d * d); DALLOC(q.wq_t, d * d);
            DALLOC(q.wup, hid * d); DALLOC(q.wup_t, hid * d); DALLOC(q.wdown, hid * d); DALLOC(q.wdown_t, hid * d);
            DALLOC(q.x1, M * d); DALLOC(q.x2, M * d); DALLOC(q.x3, M * d); DALLOC(q.st1, M); DALLOC(q.st2, M); DALLOC(q.st3, M);
            DALLOC(q.a1, M * d); DALLOC(q.a2, M * d); DALLOC(q.a3, M * d); DALLOC(q.qk, M * 2 * d); DALLOC(q.vt, M * d); DALLOC(q.att, M * d);
            DALLOC(q.qc, M * d); DALLOC(q.cr, M * d); DALLOC(q.h, M * hid); DALLOC(q.hc, M * hid); DALLOC(q.gl, M * hid); DALLOC(q.o, M * d);
            q.kvc = e->kvc_all + (size_t)i * B * 2 * 2 * d; DALLOC(q.p0, M * e->H); DALLOC(q.dww_t, 9 * hid);
        }
        return 0;
    };
    if (int rc = alloc_all()) return cleanup(rc);
    if (hipMemset(e->zero_bias, 0, e->ws.zero_bias * 4) != hipSuccess) return cleanup(fail(TLD_ERR_HIP, "hipMemset failed"));
    // angular_speeds = 2 pi exp(linspace(log 1, log 1000, ne / 2))   (tld/transformer_blocks.py:11-15; float32 arithmetic as torch does it)
    {
        const int half = e->ne / 2;
        std::vector<float> a(half);
        const float lo = logf(1.0f), hiv = logf(1000.0f);
        const float step = half > 1 ? (hiv - lo) / (float)(half - 1) : 0.f;
        for (int k = 0; k < half; ++k) {
            // torch.linspace fills the upper half from the end (hi - step * (n - 1 - k)) for symmetry
            const float v = k < half / 2 ? lo + step * (float)k : hiv - step * (float)(half - 1 - k);
            a[k] = 2.0f * 3.14159265358979323846f * expf(v);
        }
        if (hipMemcpy(e->angular, a.data(), half * 4, hipMemcpyHostToDevice) != hipSuccess) return cleanup(fail(TLD_ERR_HIP, "hipMemcpy failed"));
    }
    *out = e;
    return TLD_OK;
}

int64_t tld_train_param_count(const tld_train* e) { return e ? e->nparam : 0; }
int32_t tld_train_tensor_count(const tld_train* e) { return e ? (int32_t)e->layout.size() : 0; }

int tld_train_param_layout(const tld_train* e, int32_t index, char* key_out, int32_t key_cap, int64_t* offset, int64_t* numel) {
    if (!e || index < 0 || index >= (int32_t)e->layout.size() || !key_out || key_cap <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    const Tensor& t = e->layout[index];
    snprintf(key_out, (size_t)key_cap, "%s", t.key.c_str());
    if (offset) *offset = t.off;
    if (numel) *numel = t.numel;
    return TLD_OK;
}

/* The sinusoid buffer "fourier_feats.0.angular_speeds" is a registered buffer of the reference, not a parameter; a checkpoint's
 * values can be installed here (host fp32 [noise_embed_dims / 2]); the default is the constructor's formula. */
int tld_train_set_angular_speeds(tld_train* e, const float* host, int32_t n) {
    if (!e || !host || n != e->ne / 2) return fail(TLD_ERR_SHAPE, "angular_speeds must have %d entries", e ? e->ne / 2 : 0);
    DeviceGuard dg(e->cfg.device_id);
    HIP_TRY(hipMemcpy(e->angular, host, (size_t)n * 4, hipMemcpyHostToDevice));
    return TLD_OK;
}

int tld_train_bind(tld_train* e, float* params, float* grads) {
    if (!e || !params || !grads) return fail(TLD_ERR_INVALID, "null argument");
    e->params = params; e->grads = grads; e->weights_fresh = false;
    return TLD_OK;
}

int tld_train_refresh_weights(tld_train* e, void* hip_stream) {
    if (!e || !e->params) return fail(TLD_ERR_STATE, "tld_train_bind first");
    DeviceGuard dg(e->cfg.device_id);
    if (int rc = refresh_operands(e, e->params, reinterpret_cast<hipStream_t>(hip_stream))) return rc;
    e->weights_fresh = true;
    return TLD_OK;
}

int tld_train_forward_backward(tld_train* e, const float* x_noisy, const float* noise_level, const float* label, const float* target,
                               int32_t batch, float* loss_out, float* pred_out, void* hip_stream) {
    return tld_train_forward_backward_cb(e, x_noisy, noise_level, label, target, batch, loss_out, pred_out, hip_stream, nullptr, nullptr);
}

int tld_train_forward_backward_cb(tld_train* e, const float* x_noisy, const float* noise_level, const float* label, const float* target,
                                  int32_t batch, float* loss_out, float* pred_out, void* hip_stream, tld_grad_ready_fn grad_ready, void* user) {
    if (!e || !x_noisy || !noise_level || !label || !target || !loss_out || !pred_out) return fail(TLD_ERR_INVALID, "null argument");
    if (!e->params) return fail(TLD_ERR_STATE, "tld_train_bind first");
    if (batch <= 0 || batch > e->max_batch) return fail(TLD_ERR_INVALID, "batch %d outside [1, max_batch = %d]", batch, e->max_batch);
    DeviceGuard dg(e->cfg.device_id);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (!e->weights_fresh) { if (int rc = tld_train_refresh_weights(e, hip_stream)) return rc; }
    const int d = e->d, hid = e->hid, pd = e->pd, N = e->N, H = e->H, B = batch, M = B * N, G = e->G;
    float* P = e->params; float* Gd = e->grads;
    const dim3 blk(256);
    const int nchunk = (M + 255) / 256;
    const TrainStepPlan& plan = step_plan(e, B);
    if (e->debug) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone)
            return fail(TLD_ERR_STATE, "a debug step (tld_train_set_debug) cannot be captured into a graph");
        if (int rc = debug_begin(e, B, s)) return rc;
    }
    // the two small fp32 products of the backward on the tiled kernel (see tld_train_kernels.h)
    auto lin_dx = [&](const float* dyp, int ldy, const float* W, float* dx, int ldx, int R, int Nn, int K, int acc) {      // dx[r, k] (+)= sum_n dy[r, n] W[n, k]
        hipLaunchKernelGGL(tiled_f32_kernel, dim3((K + 31) / 32, (R + 31) / 32), dim3(256), 0, s, dyp, (long)ldy, 1L, W, 1L, (long)K, (const float*)nullptr, dx, ldx, R, K, Nn,
                           (float*)nullptr, 0, acc);
    };
    auto lin_dw = [&](const float* dyp, int ldy, const float* x, int ldx, float* dW, float* db, int R, int Nn, int K) {     // dW[n, k] = sum_r dy[r, n] x[r, k]; db[n]
        hipLaunchKernelGGL(tiled_f32_kernel, dim3((K + 31) / 32, (Nn + 31) / 32), dim3(256), 0, s, dyp, 1L, (long)ldy, x, 1L, (long)ldx, (const float*)nullptr, dW, K, Nn, K, R,
                           (float*)nullptr, 0, 0);
        if (db) hipLaunchKernelGGL(small_colsum, g1(Nn), dim3(256), 0, s, dyp, ldy, db, R, Nn, 0);
    };
    const long blk_stride = e->L > 1 ? (long)(e->lp[1].kv - e->lp[0].kv) : 0;       // (as in train_forward: block i's kv_linear.weight and its (k | v) rows)
    const long kv_stride = (long)e->max_batch * 2 * 2 * d;

    // ================================================ forward ================================================
    if (int rc = train_forward(e, P, x_noisy, noise_level, label, target, B, loss_out, pred_out, s)) return rc;

    // ================================================ backward ===============================================
    if (e->debug) for (int i = 0; i < e->L; ++i) SNAP("blk" + std::to_string(i) + ".gl", e->lb[i].gl, ST_BF16, s, M, hid);       // (the backward writes dh there)
    auto reduce = [&](int nparts, size_t stride, size_t part_off, float* dst, int n, int acc) {
        hipLaunchKernelGGL(reduce_partials, dim3((n + 15) / 16), dim3(1024), 0, s, e->part + part_off, nparts, stride, dst, n, acc);
    };
    // dW[Nn, K] = dy^T x over the M rows (dy fp32 [M, Nn], Nn = patch_dim; x [M, K]) -> dst (fixed-order sum of per-chunk partials)
    auto tall_dw = [&](const TallDwPlan& t, const float* dyp, auto xp, float* dst) {
        using TX = std::remove_cv_t<std::remove_pointer_t<decltype(xp)>>;
        const int K = t.K, nc64 = (M + 63) / 64;
        const dim3 grid((K + 255) / 256, nc64);
        switch (t.nn) {
        case 16: PATH(PB_TALL_COLS); hipLaunchKernelGGL((tall_dw_cols_partial<TX, 16>), grid, blk, 0, s, dyp, xp, K, M, 64, e->part); reduce(nc64, (size_t)16 * K, 0, dst, 16 * K, 0); break;
        case 32: PATH(PB_TALL_COLS); hipLaunchKernelGGL((tall_dw_cols_partial<TX, 32>), grid, blk, 0, s, dyp, xp, K, M, 64, e->part); reduce(nc64, (size_t)32 * K, 0, dst, 32 * K, 0); break;
        case 64: PATH(PB_TALL_COLS); hipLaunchKernelGGL((tall_dw_cols_partial<TX, 64>), grid, blk, 0, s, dyp, xp, K, M, 64, e->part); reduce(nc64, (size_t)64 * K, 0, dst, 64 * K, 0); break;
        default:
            PATH(PB_TALL_PART);
            hipLaunchKernelGGL((tall_dw_partial<TX>), dim3((pd * K + 255) / 256, nchunk), blk, 0, s, dyp, pd, xp, K, M, 256, e->part);
            reduce(nchunk, (size_t)pd * K, 0, dst, pd * K, 0);
            break;
        }
    };
    // LayerNorm backward over `rows` rows of width d
    auto ln_bwd_rows = [&](auto dyp, auto xp, const float2* st, const float* gamma, float* dx, int acc, float* dgamma, float* dbeta, int rows, bf16* dxb = nullptr) {
        using TDY = std::remove_cv_t<std::remove_pointer_t<decltype(dyp)>>;
        using TX = std::remove_cv_t<std::remove_pointer_t<decltype(xp)>>;
        const int width = d, nb = (rows + 31) / 32;                       // 32 rows per workgroup: >= 1024 workgroups at the training batch
        switch (plan.lnb_q4) {
        case 3: PATH(PB_LNB_Q4 + 2); hipLaunchKernelGGL((ln_bwd_q4_kernel<TDY, TX, 3>), dim3(nb), blk, 0, s, dyp, xp, st, gamma, dx, acc, e->part, 32, rows, dxb); break;
        case 2: PATH(PB_LNB_Q4 + 1); hipLaunchKernelGGL((ln_bwd_q4_kernel<TDY, TX, 2>), dim3(nb), blk, 0, s, dyp, xp, st, gamma, dx, acc, e->part, 32, rows, dxb); break;
        case 1: PATH(PB_LNB_Q4); hipLaunchKernelGGL((ln_bwd_q4_kernel<TDY, TX, 1>), dim3(nb), blk, 0, s, dyp, xp, st, gamma, dx, acc, e->part, 32, rows, dxb); break;
        default: PATH(PB_LNB_GEN); hipLaunchKernelGGL((ln_bwd_kernel<TDY, TX>), dim3(nb), blk, 0, s, dyp, xp, st, gamma, dx, acc, e->part, 32, rows, width, dxb); break;
        }
        if (dbeta == dgamma + width) reduce(nb, 2 * (size_t)width, 0, dgamma, 2 * width, 0);       // (weight, bias) are neighbours in the flat vector: one launch
        else {
            reduce(nb, 2 * (size_t)width, 0, dgamma, width, 0);
            reduce(nb, 2 * (size_t)width, width, dbeta, width, 0);
        }
    };
    // column sums of the M rows of a [M, c.cols] matrix
    auto colsum = [&](const ColsumPlan& c, auto ap, float* dst) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(ap)>>;
        const int rows = M, cols = c.cols;
        if (c.four) {
            const int nb = (rows + 63) / 64;
            PATH(PB_COLSUM4);
            hipLaunchKernelGGL((colsum4_partial<T>), dim3((cols / 4 + 255) / 256, nb), blk, 0, s, ap, rows, cols, 64, e->part);
            reduce(nb, (size_t)cols, 0, dst, cols, 0);
        } else {
            const int nb = (rows + 255) / 256;
            PATH(PB_COLSUM);
            hipLaunchKernelGGL((colsum_partial<T>), dim3((cols + 255) / 256, nb), blk, 0, s, ap, rows, cols, 256, e->part);
            reduce(nb, (size_t)cols, 0, dst, cols, 0);
        }
    };
    // dW[Nout, Kin] = dY^T X with dY [M, Nout], X [M, Kin] (bf16), in the form and with the split the plan chose (wgrad_plan, tld_train_plan.h).  The
    // transposing forms write both operands transposed so that the contraction (M) is contiguous: the stacked operands [split][Nout | Kin][run_rows], ONE GEMM
    // launch multiplies every split with its own W block (GemmParams::w_batch_rows) into fp32 partials [split][Nout][Kin], and a fixed-order sum finishes
    // (bit-reproducible).
    auto weight_grad = [&](const WgradPlan& w, const bf16* dY, int Nout, const bf16* X, int Kin, float* dW) -> int {
        const int sk = w.sk, ms = w.run_rows;
        auto tr64 = [&](const bf16* src, int cols, bf16* dst) { hipLaunchKernelGGL(transpose_bf16_64, dim3(cols / 64, sk * ms / 64), blk, 0, s, src, cols, dst, ms, M, cols, sk); };
        switch (w.form) {
        case WG_TN:
            PATH(PB_WG_TN);
            wgrad_tn(dY, Nout, X, Kin, M, WgradSplit{sk, ms}, dW, e->splitk, s);
            return 0;
        case WG_PAD:       // the GEMM's K loop takes whole 64-row steps: the transposed operands get zero columns up to the next multiple of 64 (one run)
            PATH(PB_WG_PAD);
            hipMemsetAsync(e->T1, 0, (size_t)Nout * ms * 2, s);
            hipMemsetAsync(e->T2, 0, (size_t)Kin * ms * 2, s);
            hipLaunchKernelGGL((transpose_to_bf16<bf16>), dim3((Nout + 31) / 32, (M + 31) / 32), blk, 0, s, dY, Nout, e->T1, ms, M, Nout, sk);
            hipLaunchKernelGGL((transpose_to_bf16<bf16>), dim3((Kin + 31) / 32, (M + 31) / 32), blk, 0, s, X, Kin, e->T2, ms, M, Kin, sk);
            return gemm_f32(e->T1, ms, e->T2, ms, dW, Nout, Kin, ms, s);
        case WG_TR1:
            PATH(PB_WG_TR1);
            tr64(dY, Nout, e->T1); tr64(X, Kin, e->T2);
            return gemm_f32(e->T1, ms, e->T2, ms, dW, Nout, Kin, ms, s);
        default: {
            PATH(PB_WG_TRSK);
            tr64(dY, Nout, e->T1); tr64(X, Kin, e->T2);
            GemmParams g{};
            g.A = e->T1; g.lda = ms; g.W = e->T2; g.ldw = ms; g.M = sk * Nout; g.N = Kin; g.K = ms; g.c_f32 = e->splitk; g.ldc = Kin;
            g.w_batch_rows = Nout; g.w_batch_stride_bytes = (unsigned)((size_t)Kin * ms * 2);
            if (int rc = launch_gemm(g, EPI_F32, s)) return rc;
            hipLaunchKernelGGL(sum_slices, dim3((unsigned)(((size_t)Nout * Kin / 4 + 255) / 256)), blk, 0, s, e->splitk, sk, (size_t)Nout * Kin, dW, (size_t)Nout * Kin / 4);
            return 0;
        }
        }
    };

    // out_proj: gx = dout Wout;  dWout = dout^T x_final;  dbout
    // gx and its bf16 copy (the top block's GEMM operand)
    switch (plan.tail4) {
    case 16: PATH(PB_TAIL4_16); hipLaunchKernelGGL((tail_dx4_kernel<16>), g1((size_t)M * d / 4), blk, 0, s, e->dout, P + e->outw, e->gx, e->gxb, M, d); break;
    case 32: PATH(PB_TAIL4_32); hipLaunchKernelGGL((tail_dx4_kernel<32>), g1((size_t)M * d / 4), blk, 0, s, e->dout, P + e->outw, e->gx, e->gxb, M, d); break;
    case 64: PATH(PB_TAIL4_64); hipLaunchKernelGGL((tail_dx4_kernel<64>), g1((size_t)M * d / 4), blk, 0, s, e->dout, P + e->outw, e->gx, e->gxb, M, d); break;
    default: PATH(PB_TAIL_GEN); hipLaunchKernelGGL(tail_dx_kernel, g1((size_t)M * d), blk, 0, s, e->dout, P + e->outw, e->gx, e->gxb, M, pd, d); break;
    }
    SNAP("gx.tail", e->gx, ST_F32, s, M, d); SNAP("gxb.tail", e->gxb, ST_BF16, s, M, d);
    tall_dw(plan.tall[TALL_OUT], e->dout, (const bf16*)e->xfin, Gd + e->outw);
    colsum(plan.colsum[CS_PD], e->dout, Gd + e->outb);

    for (int i = e->L - 1; i >= 0; --i) {
        LayerB& b = e->lb[i]; const LayerP& p = e->lp[i];
        const std::string sn = e->debug ? "blk" + std::to_string(i) + "." : std::string();
        SNAP(sn + "gx.in", e->gx, ST_F32, s, M, d);
        // ---- MLP: o = g Wdown^T + b;  g = GELU(hc);  hc = dwconv(h);  h = a3 Wup^T + b;  a3 = LN3(x3)
        // (e->gxb = bf16(e->gx): written by whoever completed gx -- tail_dx_kernel for the top block, the LayerNorm-1 backward of the block above otherwise)
        colsum(plan.colsum[CS_D], e->gxb, Gd + p.down_b);
        GEMM_TRY("training step", weight_grad(plan.wg[WGP_DOWN], e->gxb, d, b.gl, hid, Gd + p.down_w));
        GEMM_TRY("training step", gemm_bf16(e->gxb, d, b.wdown_t, d, e->zero_bias, e->dbig, M, hid, d, s));                         // dg = go Wdown
        SNAP(sn + "dg", e->dbig, ST_BF16, s, M, hid);
        if (plan.dw_fused) {      PATH(PB_DW_FUSED);      // GELU' multiply, depthwise weight-gradient partials and input gradient in one pass (both images of a (sample, 64-channel chunk) in LDS)
            hipLaunchKernelGGL(dwconv_bwd_img_kernel, dim3(plan.dw_bwd_grid), blk, plan.dw_bwd_lds, s, e->dbig, b.hc, b.h, b.dww_t, b.gl, e->part, G, hid);   // dh -> b.gl (its forward value is consumed)
            hipLaunchKernelGGL(dwconv_wgrad_reduce, dim3((hid * 11 + 63) / 64), dim3(1024), 0, s, e->part, Gd + p.dw_w, Gd + p.dw_b, B, hid, 11, Gd + p.up_b);   // + the up-projection's bias gradient
        } else {
            PATH(PB_DW_UNFUSED);
            hipLaunchKernelGGL(gelu_bwd_kernel, g1((size_t)M * hid / 8), blk, 0, s, e->dbig, b.hc, e->dbig, (size_t)M * hid / 8);      // dhc (in place); b.hc = GELU'(pre-activation)
            SNAP(sn + "dhc", e->dbig, ST_BF16, s, M, hid);
            hipLaunchKernelGGL(dwconv_wgrad_kernel, dim3((hid + 255) / 256, B * G), blk, 0, s, e->dbig, b.h, e->part, G, hid);
            hipLaunchKernelGGL(dwconv_wgrad_reduce, dim3((hid * 10 + 63) / 64), dim3(1024), 0, s, e->part, Gd + p.dw_w, Gd + p.dw_b, B * G, hid);
            hipLaunchKernelGGL(dwconv_kernel, dim3(plan.dw_grid), blk, plan.dw_lds, s, e->dbig, b.dww_t, (const float*)nullptr, b.gl, (bf16*)nullptr, B, G, hid, 1, plan.dw_rows);   // dh -> b.gl
        }
        SNAP(sn + "dh", b.gl, ST_BF16, s, M, hid);
        if (plan.colsum[CS_HID].used) colsum(plan.colsum[CS_HID], b.gl, Gd + p.up_b);
        GEMM_TRY("training step", weight_grad(plan.wg[WGP_UP], b.gl, hid, b.a3, d, Gd + p.up_w));
        GEMM_TRY("training step", gemm_bf16(b.gl, hid, b.wup_t, hid, e->zero_bias, e->dsmall2, M, d, hid, s));                     // da3 = dh Wup
        SNAP(sn + "da3", e->dsmall2, ST_BF16, s, M, d);
        ln_bwd_rows(e->dsmall2, b.x3, b.st3, P + p.n3w, e->gx, 1, Gd + p.n3w, Gd + p.n3b, M);
        SNAP(sn + "gx.ln3", e->gx, ST_F32, s, M, d);
        // ---- cross-attention: cr = CA(qc, kv);  qc = a2 Wq^T;  kv = y Wkv^T;  a2 = LN2(x2)
        float* dkv = e->dkv_all + (size_t)i * kv_stride;
        hipLaunchKernelGGL(cross_bwd_kernel, dim3(B * H), blk, 0, s, e->gx, b.qc, b.kvc, b.p0, e->dsmall2, dkv, N, d);   // dqc -> dsmall2
        SNAP(sn + "dqc", e->dsmall2, ST_BF16, s, M, d); SNAP(sn + "dkv", dkv, ST_F32, s, 2 * B, 2 * d);
        lin_dw(dkv, 2 * d, e->y, d, Gd + p.kv, nullptr, 2 * B, 2 * d, d);       // (per block: its gradient range must be complete at the grad_ready call below)
        GEMM_TRY("training step", weight_grad(plan.wg[WGP_Q], e->dsmall2, d, b.a2, d, Gd + p.q));
        GEMM_TRY("training step", gemm_bf16(e->dsmall2, d, b.wq_t, d, e->zero_bias, e->dsmall, M, d, d, s));                       // da2 = dqc Wq
        SNAP(sn + "da2", e->dsmall, ST_BF16, s, M, d);
        ln_bwd_rows(e->dsmall, b.x2, b.st2, P + p.n2w, e->gx, 1, Gd + p.n2w, Gd + p.n2b, M);
        SNAP(sn + "gx.ln2", e->gx, ST_F32, s, M, d);
        // ---- self-attention: att = SDPA(q, k, v);  qkv = a1 Wqkv^T;  a1 = LN1(x1)
        int attn_path = 0;
        if (launch_attention_bwd(b.qk, b.vt, b.att, e->gx, e->dsmall, e->attn_stats, B, N, H, s, &attn_path)) return fail(TLD_ERR_INVALID, "attention backward: unsupported token count %d", N);
        if (attn_path & 1) PATH(PB_ATT_ONE);
        if (attn_path & 2) PATH(PB_ATT_TWO);
        if (attn_path & 4) PATH(PB_ATT_MASKED);
        SNAP(sn + "dqkv", e->dsmall, ST_BF16, s, M, 3 * d);
        // (dO as a bf16 copy from the LayerNorm-2 backward: 192 -> 189 us, but delta = dO . O from rounded dO moves the worst g15 gradient from 1.86e-2 to 1.92e-2 of a 2e-2 bound: not taken)
        GEMM_TRY("training step", weight_grad(plan.wg[WGP_QKV], e->dsmall, 3 * d, b.a1, d, Gd + p.qkv));
        GEMM_TRY("training step", gemm_bf16(e->dsmall, 3 * d, b.wqkv_t, 3 * d, e->zero_bias, e->dsmall2, M, d, 3 * d, s));         // da1 = dqkv Wqkv
        SNAP(sn + "da1", e->dsmall2, ST_BF16, s, M, d);
        ln_bwd_rows(e->dsmall2, b.x1, b.st1, P + p.n1w, e->gx, 1, Gd + p.n1w, Gd + p.n1b, M, i > 0 ? e->gxb : nullptr);
        SNAP(sn + "gx.ln1", e->gx, ST_F32, s, M, d);
        if (i > 0) SNAP(sn + "gxb.ln1", e->gxb, ST_BF16, s, M, d);
        // every gradient of this block is enqueued (its 15 tensors are one contiguous range of the flat vector): the data-parallel
        // reduction of that slice can start now, under the backward of the blocks below
        if (grad_ready) grad_ready(user, p.qkv, (p.n3b + d) - p.qkv);
    }
    // dL/dy = sum over blocks of dkv_i Wkv_i: one batched launch into per-block parts, then a fixed-order sum
    hipLaunchKernelGGL(tiled_f32_kernel, dim3((d + 31) / 32, (2 * B + 31) / 32, e->L), dim3(256), 0, s, e->dkv_all, (long)(2 * d), 1L, P + e->lp[0].kv, 1L, (long)d,
                       (const float*)nullptr, e->dy_parts, d, 2 * B, d, 2 * d, (float*)nullptr, 0, 0, kv_stride, blk_stride, (long)e->max_batch * 2 * d);
    hipLaunchKernelGGL(reduce_partials, dim3((2 * B * d + 15) / 16), dim3(1024), 0, s, e->dy_parts, e->L, (size_t)e->max_batch * 2 * d, e->dy, 2 * B * d, 0);
    // ---- patch embedding: x0 = LN2(e) + pos;  e = pn Wlin^T + b;  pn = LN1(p);  p = conv(x)     (tld/denoiser.py:34-45,75-77)
    SNAP("dy", e->dy, ST_F32, s, 2 * B, d);
    hipLaunchKernelGGL(pos_grad_kernel, g1((size_t)N * d), blk, 0, s, e->gx, Gd + e->pos, B, N, d);
    ln_bwd_rows(e->gx, e->e, e->est2, P + e->l2w, e->de, 0, Gd + e->l2w, Gd + e->l2b, M);
    SNAP("de", e->de, ST_F32, s, M, d);
    colsum(plan.colsum[CS_D], e->de, Gd + e->lib);
    lin_dx(e->de, d, P + e->liw, e->dpn, pd, M, d, pd, 0);               // dpn = de Wlin
    SNAP("dpn", e->dpn, ST_F32, s, M, pd);
    tall_dw(plan.tall[TALL_LIN], e->p16n, (const float*)e->de, e->scr);                                                                              // dWlin^T [pd, d]
    hipLaunchKernelGGL(transpose_f32_small, g1((size_t)pd * d), blk, 0, s, e->scr, Gd + e->liw, pd, d);
    hipLaunchKernelGGL(ln_small_bwd_kernel, dim3(nchunk), blk, 0, s, e->dpn, e->p16, e->est1, P + e->l1w, e->dp16, e->part, M, pd);
    SNAP("dp16", e->dp16, ST_F32, s, M, pd);
    reduce(nchunk, 2 * (size_t)pd, 0, Gd + e->l1w, pd, 0);
    reduce(nchunk, 2 * (size_t)pd, pd, Gd + e->l1b, pd, 0);
    hipLaunchKernelGGL(patches_kernel, g1((size_t)M * pd), blk, 0, s, x_noisy, e->patches, B, e->C, e->S, e->cfg.patch_size, G);
    tall_dw(plan.tall[TALL_CONV], e->dp16, (const float*)e->patches, Gd + e->cvw);
    colsum(plan.colsum[CS_PD], e->dp16, Gd + e->cvb);
    // ---- conditioning: y = LN(stack[nz, lb]);  nz = W3 GELU(W1 sin + b1) + b3;  lb = label_proj(label)     (tld/denoiser.py:105-122)
    ln_bwd_rows(e->dy, e->ycat, e->yst, P + e->nw, e->dycat, 0, Gd + e->nw, Gd + e->nb, 2 * B);
    SNAP("dycat", e->dycat, ST_F32, s, 2 * B, d);
    lin_dw(e->dycat + d, 2 * d, label, e->text, Gd + e->lbw, Gd + e->lbb, B, d, e->text);
    lin_dw(e->dycat, 2 * d, e->g1v, d, Gd + e->ff3w, Gd + e->ff3b, B, d, d);
    lin_dx(e->dycat, 2 * d, P + e->ff3w, e->dg1, d, B, d, d, 0);
    hipLaunchKernelGGL(mul_gelu_grad, g1((size_t)B * d), blk, 0, s, e->dg1, e->h1, B * d);
    SNAP("dg1", e->dg1, ST_F32, s, B, d);
    lin_dw(e->dg1, d, e->sinb, e->ne, Gd + e->ff1w, Gd + e->ff1b, B, d, e->ne);
    if (grad_ready) {       // the ranges around the blocks: conditioning MLP / patch embedding / position table; out_proj, norm, label_proj
        grad_ready(user, 0, e->lp[0].qkv);
        grad_ready(user, e->outw, e->nparam - e->outw);
    }
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* The forward half of tld_train_forward_backward on any flat weight vector (include/tld_hip.h): train_forward, then the per-sample reduction.
 * Writes no gradient, calls nothing back, advances nothing. */
int tld_train_forward_loss(tld_train* e, const float* weights, const float* x_noisy, const float* noise_level, const float* label, const float* target,
                           int32_t batch, float* loss_out, double* sample_loss_out, float* pred_out, void* hip_stream) {
    if (!e || !x_noisy || !noise_level || !label || !target || !loss_out) return fail(TLD_ERR_INVALID, "forward loss: null argument");
    if (batch <= 0 || batch > e->max_batch) return fail(TLD_ERR_INVALID, "forward loss: batch %d outside [1, max_batch = %d]", batch, e->max_batch);
    if (sample_loss_out && ((uintptr_t)sample_loss_out & 7)) return fail(TLD_ERR_INVALID, "forward loss: sample_loss_out must be 8-byte aligned");
    if (!e->params) return fail(TLD_ERR_STATE, "tld_train_bind first");
    if (e->debug) return fail(TLD_ERR_STATE, "forward loss: the stage hook is on (tld_train_set_debug): a debug call poisons the gradient vector, which this entry never writes");
    DeviceGuard dg(e->cfg.device_id);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const bool bound = !weights || weights == e->params;
    const float* P = bound ? e->params : weights;
    if (!bound) {
        e->weights_fresh = false;                                        // (first: an error below must not leave foreign operand copies marked fresh)
        if (int rc = refresh_operands(e, P, s)) return rc;
    } else if (!e->weights_fresh) {
        if (int rc = refresh_operands(e, P, s)) return rc;
        e->weights_fresh = true;
    }
    if (int rc = train_forward(e, P, x_noisy, noise_level, label, target, batch, loss_out, pred_out ? pred_out : e->pred_scratch, s)) return rc;
    if (sample_loss_out) {
        if (int rc = tld_train_sample_loss(e, nullptr, batch, 0, 0, sample_loss_out, hip_stream)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* out[b] = (sum of the rows of sample b) / elems_per_sample in double, fixed order (sample_loss_kernel). */
int tld_train_sample_loss(tld_train* e, const float* row_sq, int32_t batch, int32_t rows_per_sample, int64_t elems_per_sample, double* out, void* hip_stream) {
    if (!out || ((uintptr_t)out & 7)) return fail(TLD_ERR_INVALID, "sample loss: out is null or not 8-byte aligned");
    if (batch <= 0) return fail(TLD_ERR_INVALID, "sample loss: batch %d", batch);
    if (!row_sq) {
        if (!e) return fail(TLD_ERR_INVALID, "sample loss: neither rows nor an engine");
        if (e->last_batch == 0) return fail(TLD_ERR_STATE, "sample loss: the engine has run no forward yet");
        if (batch != e->last_batch && batch != e->captured_batch)
            return fail(TLD_ERR_STATE, "sample loss: batch %d, but the engine's last forward had %d samples", batch, e->last_batch);
        row_sq = e->row_loss; rows_per_sample = e->N; elems_per_sample = (int64_t)e->C * e->S * e->S;
    } else if (rows_per_sample <= 0 || elems_per_sample <= 0) {
        return fail(TLD_ERR_INVALID, "sample loss: rows_per_sample %d, elems_per_sample %lld", rows_per_sample, (long long)elems_per_sample);
    }
    DeviceGuard dg(e ? e->cfg.device_id : std::max(0, ptr_device(out)));
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    if (rows_per_sample <= 1024)
        hipLaunchKernelGGL((sample_loss_kernel<true>), dim3(((unsigned)batch + 3) / 4), dim3(256), 0, s, row_sq, batch, rows_per_sample, (double)elems_per_sample, out);
    else
        hipLaunchKernelGGL((sample_loss_kernel<false>), dim3((unsigned)batch), dim3(256), 0, s, row_sq, batch, rows_per_sample, (double)elems_per_sample, out);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* The accumulator by noise level (state layout: include/tld_hip.h); one workgroup, serial per bucket (loss_buckets_kernel). */
int tld_train_loss_buckets(const double* sample_loss, const float* noise_level, int32_t batch, int32_t n_buckets, double* state, void* hip_stream) {
    if (!sample_loss || !noise_level || !state) return fail(TLD_ERR_INVALID, "loss buckets: null pointer");
    if (((uintptr_t)state & 7) || ((uintptr_t)sample_loss & 7)) return fail(TLD_ERR_INVALID, "loss buckets: state and sample_loss must be 8-byte aligned");
    if (n_buckets < 1 || n_buckets > LOSS_BUCKETS_MAX) return fail(TLD_ERR_INVALID, "loss buckets: n_buckets %d outside [1, %d]", n_buckets, LOSS_BUCKETS_MAX);
    if (batch < 1) return fail(TLD_ERR_INVALID, "loss buckets: batch %d", batch);
    DeviceGuard dg(std::max(0, ptr_device(state)));
    hipLaunchKernelGGL(loss_buckets_kernel, dim3(1), dim3(LOSS_BUCKETS_THREADS), 0, reinterpret_cast<hipStream_t>(hip_stream), sample_loss, noise_level, batch, n_buckets,
                       state);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* optimizer.step() of torch.optim.Adam(model.parameters(), lr) (tld/train.py:87,169) fused with update_ema (tld/train.py:55-58,172) over
 * flat fp32 device vectors; step counts from 1.  ema may be NULL (ranks other than the main process hold no EMA copy, :110-112).
 * grad_scale multiplies the gradient first (1 / world_size after a SUM all-reduce). */
int tld_train_adam_ema(tld_train* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr,
                       float beta1, float beta2, float eps, int32_t step, float ema_alpha, float grad_scale, void* hip_stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || numel <= 0 || step <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    DeviceGuard dg(e ? e->cfg.device_id : 0);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
    hipLaunchKernelGGL(adam_ema_kernel, g1((size_t)numel), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, ema, (size_t)numel, lr, beta1, beta2, eps, bc1, bc2,
                       ema_alpha, grad_scale);
    HIP_TRY(hipGetLastError());
    if (e && params == e->params) e->weights_fresh = false;          // the bf16 operand copies are stale now
    return TLD_OK;
}

static_assert(TLD_TRAIN_OPT_STATE_DOUBLES == GUARD_STATE_HEAD + GUARD_PARTS, "state layout of include/tld_hip.h");

/* The guard in front of tld_train_adam_ema_guarded (state layout and finalize rule: include/tld_hip.h): the global norm of grads * grad_scale
 * from 1024 fixed-order double partials (no atomics: bitwise repeatable), then clip coefficient / skip decision / Adam's step count and bias
 * corrections into opt_state, all on the stream -- the host never waits. */
int tld_train_grad_guard(tld_train* e, const float* grads, int64_t numel, float grad_scale, double max_norm, int32_t skip_nonfinite, float beta1,
                         float beta2, double* opt_state, void* hip_stream) {
    if (!grads || !opt_state) return fail(TLD_ERR_INVALID, "grad guard: null gradient or state pointer");
    if (numel <= 0) return fail(TLD_ERR_INVALID, "grad guard: numel %lld", (long long)numel);
    if (std::isnan(max_norm)) return fail(TLD_ERR_INVALID, "grad guard: max_norm is NaN (<= 0 or +inf: no clipping)");
    if (((uintptr_t)grads & 15) || ((uintptr_t)opt_state & 7))
        return fail(TLD_ERR_INVALID, "grad guard: grads must be 16-byte and opt_state 8-byte aligned");
    DeviceGuard dg(e ? e->cfg.device_id : std::max(0, ptr_device(grads)));
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)numel, chunk = ((n + GUARD_PARTS - 1) / GUARD_PARTS + 3) / 4 * 4;
    const int clip = max_norm > 0.0 && !std::isinf(max_norm);
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3(GUARD_PARTS), dim3(256), 0, s, grads, n, chunk, grad_scale, opt_state + GUARD_STATE_HEAD);
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(256), 0, s, opt_state, max_norm, clip, skip_nonfinite ? 1 : 0, beta1, beta2);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* tld_train_adam_ema with the clip coefficient and the bias corrections read from opt_state on the device; a step the guard marked skipped
 * leaves every vector as it was. */
int tld_train_adam_ema_guarded(tld_train* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr,
                               float beta1, float beta2, float eps, float ema_alpha, float grad_scale, const double* opt_state, void* hip_stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || !opt_state || numel <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    if ((uintptr_t)opt_state & 7) return fail(TLD_ERR_INVALID, "opt_state must be 8-byte aligned");
    DeviceGuard dg(e ? e->cfg.device_id : std::max(0, ptr_device(params)));
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const size_t n = (size_t)numel;
    const bool vec = !(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15);
    if (vec)
        hipLaunchKernelGGL((adam_ema_guarded_kernel<true>), g1((n + 3) / 4), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps,
                           ema_alpha, grad_scale, opt_state);
    else
        hipLaunchKernelGGL((adam_ema_guarded_kernel<false>), g1(n), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, ema, n, lr, beta1, beta2, eps, ema_alpha,
                           grad_scale, opt_state);
    HIP_TRY(hipGetLastError());
    if (e && params == e->params) e->weights_fresh = false;          // the bf16 operand copies are stale now (a skipped step rebuilds the same ones)
    return TLD_OK;
}

/* ---- the grouped optimizer step (contract: include/tld_hip.h; the cut: tld_opt_plan.h) ------------------------------------------------- */
struct tld_opt_plan {
    int device = 0;
    int64_t numel = 0, n_factors = 0;
    int32_t n_seg = 0, n_chunks = 0;
    OptChunkDev* chunks = nullptr;         // [n_chunks]
    double* part = nullptr;                // [n_chunks] partial sums of squares of the last guard call
    int32_t* seg_chunk0 = nullptr;         // [n_seg + 1]
    unsigned char* seg_frozen = nullptr;   // [n_seg]
    double* seg_sq = nullptr;              // [n_seg] per-segment sums of the last guard call
    float* lr_factors = nullptr;           // [n_factors]
};

static_assert(sizeof(tld_opt_group) == sizeof(OptGroup), "tld_opt_group of include/tld_hip.h and OptGroup of tld_opt_plan.h are one layout");

void tld_opt_plan_destroy(tld_opt_plan* p) {
    if (!p) return;
    DeviceGuard dg(p->device);
    for (void* q : {(void*)p->chunks, (void*)p->part, (void*)p->seg_chunk0, (void*)p->seg_frozen, (void*)p->seg_sq, (void*)p->lr_factors})
        if (q) (void)hipFree(q);
    delete p;
}

int tld_opt_plan_create(int32_t device, const int64_t* seg_numel, const int32_t* seg_group, int32_t n_seg, const tld_opt_group* groups, int32_t n_groups,
                        const float* lr_factors, int64_t n_factors, tld_opt_plan** out) {
    const std::string why = opt_plan_check(seg_numel, seg_group, n_seg, reinterpret_cast<const OptGroup*>(groups), n_groups, lr_factors, n_factors, out);
    if (!why.empty()) return fail(TLD_ERR_INVALID, "opt plan: %s", why.c_str());
    *out = nullptr;
    if (device < 0) return fail(TLD_ERR_INVALID, "opt plan: device %d", device);
    if (opt_chunk_count(seg_numel, n_seg) > (int64_t)1 << 30)
        return fail(TLD_ERR_INVALID, "opt plan: %lld chunks (at most 2^30)", (long long)opt_chunk_count(seg_numel, n_seg));
    const OptCut cut = opt_cut(seg_numel, n_seg);
    std::vector<OptChunkDev> rec(cut.chunks.size());
    for (size_t c = 0; c < rec.size(); ++c) {
        const OptChunk& k = cut.chunks[c];
        const tld_opt_group& q = groups[seg_group[k.seg]];
        rec[c] = OptChunkDev{(long long)k.first, k.len, k.seg, q.lr_scale, q.weight_decay, q.frozen, 0};
    }
    std::vector<int32_t> c0(cut.seg_chunk0.begin(), cut.seg_chunk0.end());
    std::vector<unsigned char> frozen((size_t)n_seg);
    for (int32_t s = 0; s < n_seg; ++s) frozen[(size_t)s] = (unsigned char)groups[seg_group[s]].frozen;
    tld_opt_plan* p = new tld_opt_plan();
    p->device = device; p->numel = cut.numel; p->n_factors = n_factors; p->n_seg = n_seg; p->n_chunks = (int32_t)rec.size();
    DeviceGuard dg(device);
    auto up = [](auto** dst, const void* src, size_t bytes) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(dst), bytes ? bytes : 16);
        if (e == hipSuccess && src && bytes) e = hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess && !src) e = hipMemset(*dst, 0, bytes ? bytes : 16);
        return e;
    };
    hipError_t e = up(&p->chunks, rec.data(), rec.size() * sizeof(OptChunkDev));
    if (e == hipSuccess) e = up(&p->part, nullptr, rec.size() * sizeof(double));
    if (e == hipSuccess) e = up(&p->seg_chunk0, c0.data(), c0.size() * sizeof(int32_t));
    if (e == hipSuccess) e = up(&p->seg_frozen, frozen.data(), frozen.size());
    if (e == hipSuccess) e = up(&p->seg_sq, nullptr, (size_t)n_seg * sizeof(double));
    if (e == hipSuccess && n_factors > 0) e = up(&p->lr_factors, lr_factors, (size_t)n_factors * sizeof(float));
    if (e != hipSuccess) {
        tld_opt_plan_destroy(p);
        return fail(TLD_ERR_HIP, "opt plan: uploading the tables failed: %s", hipGetErrorString(e));
    }
    *out = p;
    return TLD_OK;
}

int64_t tld_opt_plan_numel(const tld_opt_plan* p) { return p ? p->numel : 0; }

int tld_opt_plan_segment_sqsums(const tld_opt_plan* p, const double** device_ptr) {
    if (!p || !device_ptr) return fail(TLD_ERR_INVALID, "opt plan: null plan or result pointer");
    *device_ptr = p->seg_sq;
    return TLD_OK;
}

/* tld_train_grad_guard over the plan's chunks: one partial per chunk, per-segment sums in chunk order, the global sum over the segments that
 * are not frozen in segment order, then the finalize rule and the schedule factor -- two launches on the stream, nothing allocated. */
int tld_train_grad_guard_grouped(tld_opt_plan* p, const float* grads, int64_t numel, float grad_scale, double max_norm, int32_t skip_nonfinite,
                                 float beta1, float beta2, double* opt_state, void* hip_stream) {
    if (!p || !grads || !opt_state) return fail(TLD_ERR_INVALID, "grouped grad guard: null plan, gradient or state pointer");
    if (numel != p->numel) return fail(TLD_ERR_INVALID, "grouped grad guard: numel %lld, the plan covers %lld", (long long)numel, (long long)p->numel);
    if (std::isnan(max_norm)) return fail(TLD_ERR_INVALID, "grouped grad guard: max_norm is NaN (<= 0 or +inf: no clipping)");
    if (((uintptr_t)grads & 15) || ((uintptr_t)opt_state & 7))
        return fail(TLD_ERR_INVALID, "grouped grad guard: grads must be 16-byte and opt_state 8-byte aligned");
    DeviceGuard dg(p->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    const int clip = max_norm > 0.0 && !std::isinf(max_norm);
    hipLaunchKernelGGL(seg_sqsum_kernel, dim3((unsigned)p->n_chunks), dim3(256), 0, s, grads, p->chunks, grad_scale, p->part);
    hipLaunchKernelGGL(grouped_guard_finalize_kernel, dim3(1), dim3(OPT_FIN_THREADS), 0, s, opt_state, p->part, p->seg_chunk0, p->seg_frozen, p->seg_sq, p->n_seg,
                       p->lr_factors, (long long)p->n_factors, max_norm, clip, skip_nonfinite ? 1 : 0, beta1, beta2);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* AdamW + EMA by group behind the grouped guard: one workgroup per chunk of the plan. */
int tld_train_adamw_ema_grouped(tld_opt_plan* p, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel, float lr,
                                float beta1, float beta2, float eps, float ema_alpha, float grad_scale, const double* opt_state, void* hip_stream) {
    if (!p || !params || !grads || !exp_avg || !exp_avg_sq || !opt_state) return fail(TLD_ERR_INVALID, "grouped adamw: null plan, vector or state pointer");
    if (numel != p->numel) return fail(TLD_ERR_INVALID, "grouped adamw: numel %lld, the plan covers %lld", (long long)numel, (long long)p->numel);
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15)
        return fail(TLD_ERR_INVALID, "grouped adamw: params, grads, exp_avg, exp_avg_sq and ema must be 16-byte aligned");
    if ((uintptr_t)opt_state & 7) return fail(TLD_ERR_INVALID, "grouped adamw: opt_state must be 8-byte aligned");
    DeviceGuard dg(p->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(hip_stream);
    hipLaunchKernelGGL(adamw_ema_grouped_kernel, dim3((unsigned)p->n_chunks), dim3(256), 0, s, params, grads, exp_avg, exp_avg_sq, ema, p->chunks, lr, beta1, beta2,
                       eps, ema_alpha, grad_scale, opt_state);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* Test hook: backward of softmax(Q K^T / 8) V for `batch` samples x `heads` heads over `ntok` tokens (a multiple of 16).
 * qk [M, 2 d] bf16 (q | k), vt [B, H, 64, ntok] bf16, o [M, d] bf16 (the forward output), g [M, d] fp32 (dL/dO); dqkv [M, 3 d] bf16 out
 * (dq | dk | dv); scratch: 2 * batch * heads * ntok floats (used when ntok > 256).  Device pointers. */
int tld_debug_attention_bwd(const void* qk, const void* vt, const void* o, const float* g, void* dqkv, float* scratch, int32_t batch, int32_t ntok,
                            int32_t heads, void* hip_stream) {
    if (!qk || !vt || !o || !g || !dqkv || batch <= 0 || heads <= 0 || ntok <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    if (const std::string bad = attention_bwd_hook_refusal(batch, ntok, heads); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    PtrDeviceGuard guard(qk);
    if (launch_attention_bwd(reinterpret_cast<const bf16*>(qk), reinterpret_cast<const bf16*>(vt), reinterpret_cast<const bf16*>(o), g,
                             reinterpret_cast<bf16*>(dqkv), scratch, batch, ntok, heads, reinterpret_cast<hipStream_t>(hip_stream)))
        return fail(TLD_ERR_INVALID, "attention backward: unsupported token count %d (or no scratch)", ntok);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

/* Test hook: the weight-gradient product dW[n_out, k_in] = dY^T X of the training step (dY [rows, n_out], X [rows, k_in] bf16 row-major, fp32 out)
 * on the transposed-operand GEMM; `slices`: fp32 workspace of slice_floats elements for the split-K partial sums.  Device pointers. */
int tld_debug_wgrad(const void* dy, const void* x, float* dw, float* slices, int64_t slice_floats, int32_t rows, int32_t n_out, int32_t k_in, void* hip_stream) {
    if (!dy || !x || !dw || !slices || rows <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    if (const std::string bad = wgrad_hook_refusal(rows, n_out, k_in); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    if (!wgrad_untransposed_takes(rows, n_out, k_in)) return fail(TLD_ERR_SHAPE, "n_out and k_in must be multiples of 256, rows a multiple of 64");
    PtrDeviceGuard guard(dy);
    wgrad_tn(reinterpret_cast<const bf16*>(dy), n_out, reinterpret_cast<const bf16*>(x), k_in, rows,
             wgrad_split(rows, n_out, k_in, device_cu_count(), kWgradUntransposed, (size_t)slice_floats, 0), dw, slices, reinterpret_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_train_set_debug(tld_train* e, int32_t enable) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    DeviceGuard dg(e->cfg.device_id);
    e->paths = 0;
    if (enable) {
        if (int rc = reserve_snapshots(e)) { e->stages.free_all(); e->debug = false; return rc; }
        e->debug = true;
    } else {
        e->debug = false;
        (void)hipDeviceSynchronize();
        e->stages.free_all();
    }
    return TLD_OK;
}

int tld_train_read_stage(tld_train* e, const char* name, float* host_out, int64_t numel, int64_t* shape_out) {
    if (!e || !name) return fail(TLD_ERR_INVALID, "null argument");
    DeviceGuard dg(e->cfg.device_id);
    return e->stages.read(name, host_out, numel, shape_out);      // (host_out null: the shape only)
}

int tld_train_debug_paths(tld_train* e, uint64_t* mask) {
    if (!e || !mask) return fail(TLD_ERR_INVALID, "null argument");
    *mask = e->paths;
    return TLD_OK;
}

int tld_train_destroy(tld_train* e) {
    if (!e) return TLD_OK;
    DeviceGuard dg(e->cfg.device_id);
    e->stages.free_all();
    for (void* p : e->allocs) hipFree(p);
    delete e;
    return TLD_OK;
}

}  // extern "C"

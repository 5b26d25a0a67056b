// tld_engine.hip -- host side of libtld_hip.so: weight image allocation (tld_refresh.hip builds them), workspace, kernel sequencing, C ABI.
//
// One engine = one device + one model.  The forward is a fixed sequence of hand-written kernels
// (7 per decoder block) enqueued on the caller's stream; the sampler prepares every conditioning
// table once (all timesteps, all prompts) and then runs embed -> blocks -> tail -> update per step
// with no host round trip.  See DESIGN.md for the data layout and per-kernel roofline notes.
#include "../../include/tld_hip.h"
#include "tld_common.h"
#include "tld_body_plan.h"
#include "tld_host.h"
#include "tld_refresh.h"
#include "tld_sample_plan.h"
#include "tld_session_plan.h"
#include "tld_tail_fold_math.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

using namespace tld;

namespace {
thread_local char g_err[512] = "";
}  // namespace
namespace tld {
void set_last_error(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
thread_local uint64_t* g_path_sink = nullptr;
}  // namespace tld
namespace {

enum KClass { KC_GEMM_QKV = 0, KC_GEMM_UP, KC_GEMM_DOWN, KC_ATTN, KC_CROSS, KC_DWCONV, KC_LN, KC_EMBED,
              KC_TAIL, KC_UPDATE, KC_COND, KC_COUNT };

}  // namespace

struct tld_engine : DeviceArena, BodyShape {      // (pad = 256: every allocation of this engine carries 256 bytes of over-read margin; d, L, H, grid, ntok, ...: body_shape(cfg))
    tld_engine() : BodyShape{} { pad = 256; }
    tld_config cfg{};
    BodySwitches sw;                    // the environment, read once at create (tld_engine_set_gemm_dtype(1) writes three of them: body_switches_set_dtype)
    BodyPlan mode;                      // this engine's mode (tld_body_plan.h): computed at create, again when a setter changes an input; what is HELD is frozen at finalize
    bool finalized = false;
    // the buffers whose existence the plan decides (finalize; split-K: tld_engine_set_low_latency).  Nothing below asks whether one is null: the plan says what runs.
    struct ModeBuffers {
        uint32_t* seam = nullptr;       // 32 x 32 grids: the seam rows of the hidden tensor between the fused up-projection and launch_dwconv_seam
        uint32_t* pair_park = nullptr;  // one slot of kPairSlotDwords per workgroup a two-head QKV + attention launch can have (plan.pair_slots)
        bf16* out_fold_hl = nullptr;    // out_proj folded into the last block's down projection: [Wout | Wout Wd] as a split bf16 pair [2][pdp][d + hid] ...
        float* out_fold_b = nullptr;    // ... and Wout bd + bo [pd] (tld_tail_fold_math.h)
        float* splitk = nullptr;        // [slices][max rows][d] fp32 slices of the low-latency down projection (it outlives its class: clearing the class frees nothing)
        int splitk_slices = 0;          // ... of the class set last (the buffer has room for at least that many)
    } mb;
    uint8_t *a8 = nullptr, *as8 = nullptr;   // fp8 mode: quantised A operand [M, hid] and its block scales [hid/128][M][4]
    std::map<std::string, HostTensor> host;

    // fp32 parameters
    float *angular = nullptr, *ff1_w = nullptr, *ff1_b = nullptr, *ff3_w = nullptr, *ff3_b = nullptr;
    float *label_w = nullptr, *label_b = nullptr, *norm_w = nullptr, *norm_b = nullptr;
    float *conv_w = nullptr, *conv_b = nullptr, *pln1_w = nullptr, *pln1_b = nullptr, *plin_wt = nullptr,
          *plin_b = nullptr, *pln2_w = nullptr, *pln2_b = nullptr, *pos = nullptr, *out_w = nullptr,
          *out_b = nullptr;
    bf16* out_w_hl = nullptr;           // out_proj weight as a split bf16 pair [2][pd][d] (tail_mfma_kernel)
    bf16* plin_w_hl = nullptr;          // patch-embedding Linear weight as a split bf16 pair [2][d][pd] (embed_mfma_kernel)
    std::vector<Layer> layers;
    const float **tab_kv_w = nullptr, **tab_q_w = nullptr, **tab_n2_w = nullptr, **tab_n2_b = nullptr;   // [L] device tables
    RefreshPlan refresh;                // tld_engine_refresh_weights: where every weight image above comes from in a flat parameter vector (built at finalize)
    int64_t nparam = 0;                 // length of that vector (tld_engine_param_count)

    // activations (sized for cfg.max_batch)
    resid_t* x = nullptr;
    resid_t* x_half = nullptr;         // patch embedding of the un-doubled batch (CFG layer-0 sharing)
    int64_t rows_cond = 0, rows_uncond = 0;     // model samples the last sampler call enqueued (tld_engine_sample_rows)
    float2* ln_stats = nullptr;        // [M][kLnSlots] row partial sums of the residual stream (embed / down GEMM -> QKV GEMM)
    float2* row_stats = nullptr;       // [M] (mean, rstd) of the residual rows, cross_row -> up-projection epilogue
    bf16 *xn = nullptr, *qk = nullptr, *vt = nullptr, *att = nullptr, *hid1 = nullptr, *hid2 = nullptr;
    float *io_x = nullptr, *io_sigma = nullptr, *io_label = nullptr, *io_out = nullptr;
    float *xt = nullptr, *x0_prev = nullptr;
    int* rows_dev = nullptr;           // tld_denoiser_forward's noise_row / label_row tables [2 max_batch]
    void* stage_host = nullptr;        // pinned staging for the samplers' host-built tables
    size_t stage_cap = 0;
    hipEvent_t stage_ev = nullptr;     // recorded after the last copy out of stage_host
    void* req_dev = nullptr;           // the samplers' tables of one call (run_sampler): step rows, start mixes, token-row indices
    size_t req_cap = 0;
    SamplePlan plan;                   // of the last sampler call: kept for its vectors, so a steady state plans without allocating them
    // the shaped guidance update (tld_sample_requests_shaped), allocated by the first call that needs them: the momentum buffer [max_batch, img], and
    // per request (P, Q) and the five sums of the step's guidance_stats_kernel launch
    float* shape_mom = nullptr;
    float2* shape_pq = nullptr;
    double* shape_sums = nullptr;
    // the sampler session open on this engine (tld_session_open), or null; its slot-major buffers [3][sess_slots][img] are kept for the next one
    tld_session* session = nullptr;
    float* sess_buf = nullptr;
    int sess_slots = 0;

    // conditioning tables (sized for cond_cap token rows)
    int cond_cap = 0;
    float *c_sigma = nullptr, *c_sin = nullptr, *c_h1 = nullptr, *c_pre = nullptr, *c_y = nullptr,
          *c_label = nullptr;
    float *c_kv = nullptr;             // [L][T][2d]
    float *c_wq = nullptr;             // [L][T][H][d]
    float *c_bwq = nullptr;            // [L][T][H]

    // debug stage capture (tld_engine_set_debug)
    bool debug = false;
    bool dbg_keep = false;             // the running body's stages are kept (debug on, and the sampler is at the debug step)
    int dbg_step = -1;                 // sampler step whose stages are kept (tld_engine_set_debug_step); < 0: every step, so the last one remains
    uint64_t paths = 0;                // launch paths of the last debug call
    StageStore stages;                 // the stage hook (tld_host.h)
    std::vector<std::pair<void*, size_t>> poison;      // activation / statistics / seam / split-K buffers a debug forward fills with 0xFF first

    // per-class event profiling
    // (event pairs come from a per-class pool that set_profile / profile_reserve fill OUTSIDE any timed region;
    // a launch only records into the next free pair)
    uint32_t prof_mask = 0;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[KC_COUNT];
    size_t prof_used[KC_COUNT] = {};
};

namespace {

int ensure_cond_capacity(tld_engine* e, int T) {
    if (T <= e->cond_cap) return TLD_OK;
    // grow-only; old tables are kept in e->allocs and freed at destroy (growth happens at most a few times)
    const int cap = ((T + 63) / 64) * 64;
    const size_t d = e->d, L = e->L, H = e->H;
    if (int rc = dev_alloc(e, &e->c_sigma, (size_t)cap)) return rc;
    if (int rc = dev_alloc(e, &e->c_sin, (size_t)cap * e->ne)) return rc;
    if (int rc = dev_alloc(e, &e->c_h1, (size_t)cap * d)) return rc;
    if (int rc = dev_alloc(e, &e->c_pre, (size_t)cap * d)) return rc;
    if (int rc = dev_alloc(e, &e->c_y, (size_t)cap * d)) return rc;
    if (int rc = dev_alloc(e, &e->c_label, (size_t)cap * e->text)) return rc;
    if (int rc = dev_alloc(e, &e->c_kv, L * cap * 2 * d)) return rc;
    if (int rc = dev_alloc(e, &e->c_wq, L * cap * H * d)) return rc;
    if (int rc = dev_alloc(e, &e->c_bwq, L * cap * H)) return rc;
    e->cond_cap = cap;
    return TLD_OK;
}

int ensure_req_capacity(tld_engine* e, size_t bytes) {
    if (bytes <= e->req_cap) return TLD_OK;
    char* q = nullptr;
    if (int rc = dev_alloc(e, &q, bytes)) return rc;      // grow-only, like the conditioning tables
    e->req_dev = q; e->req_cap = bytes;
    return TLD_OK;
}

// Pinned host staging owned by the engine: tld_sample fills it and returns without waiting for the copies; the
// next call waits on stage_ev (long complete by then) before overwriting.
int stage_acquire(tld_engine* e, size_t bytes) {
    if (!e->stage_ev) HIP_TRY(hipEventCreateWithFlags(&e->stage_ev, hipEventDisableTiming));
    else HIP_TRY(hipEventSynchronize(e->stage_ev));
    if (bytes <= e->stage_cap) return TLD_OK;
    if (e->stage_host) { HIP_TRY(hipHostFree(e->stage_host)); e->stage_host = nullptr; e->stage_cap = 0; }
    const size_t cap = (bytes + 4095) & ~(size_t)4095;
    HIP_TRY(hipHostMalloc(&e->stage_host, cap, hipHostMallocDefault));
    e->stage_cap = cap;
    return TLD_OK;
}

struct ProfScope {
    tld_engine* e; int cls; hipStream_t s; hipEvent_t b = nullptr; bool on;
    ProfScope(tld_engine* e_, int cls_, hipStream_t s_) : e(e_), cls(cls_), s(s_) {
        on = (e->prof_mask >> cls) & 1u;
        if (!on) return;
        auto& pool = e->prof_ev[cls];
        if (e->prof_used[cls] == pool.size()) {          // pool exhausted (no tld_engine_profile_reserve): grow here
            hipEvent_t a2 = nullptr, b2 = nullptr;
            hipEventCreate(&a2); hipEventCreate(&b2);
            pool.emplace_back(a2, b2);
        }
        const auto& pr = pool[e->prof_used[cls]++];
        b = pr.second;
        hipEventRecord(pr.first, s);
    }
    ~ProfScope() { if (on) hipEventRecord(b, s); }
};

// ---- stage hook (StageStore, tld_host.h): this engine's names, sizes and poison step ---------------------------------------------------
#define SNAP(...) do { if (e->dbg_keep) { if (int _r = e->stages.copy(__VA_ARGS__)) return _r; } } while (0)
inline std::string blk_name(int l, const char* n) { return "blk" + std::to_string(l) + "." + n; }

// the engine's mode from its inputs (create, the two setters); after finalize what is held stays
inline void replan(tld_engine* e, bool fp8, int cls) {
    e->mode = plan_body(*e, e->sw, fp8, cls, e->cfg.max_batch, device_cu_count(), e->finalized ? &e->mode : nullptr);
}

// set_debug(1): memory for every snapshot a forward of max_batch samples takes (the names of the SNAP calls in run_body and the samplers),
// and the names of what is read in place: the conditioning tables and the GEMM operands as the engine holds them
int reserve_snapshots(tld_engine* e) {
    const BodyPlan& P = e->mode;
    const size_t d = e->d, hid = e->hid;
    for (const BodyStage& st : body_stages(*e, P, e->cfg.max_batch, e->mb.splitk_slices))
        if (int rc = e->stages.reserve(st.name, st.bytes)) return rc;
    const std::vector<BodyImage> images = body_block_images(*e, P);
    for (int l = 0; l < e->L; ++l) {
        const Layer& Ly = e->layers[l];
        StageStore& S = e->stages;
        if (P.fused_qa) {      // rows in the fused kernel's packed order: the reader needs d and the head count to undo it
            const struct { const char* n; const void* p; int dt; int64_t cols; } packed[] = {{"wqkv", Ly.qkv_wp, ST_BF16, (int64_t)d}, {"qkv_c1", Ly.qkv_c1p, ST_F32, 1}, {"qkv_b1", Ly.qkv_b1p, ST_F32, 1}};
            for (const auto& q : packed)
                if (Stage* st = S.ref(blk_name(l, q.n), q.p, q.dt, 3 * d, q.cols, 1, 1, 0, SL_QKV_ROWS)) { st->extra.d = e->d; st->extra.heads = e->H; }
        } else {
            S.ref(blk_name(l, "wqkv"), P.fold_ln1 ? Ly.qkv_wf : Ly.qkv_w, ST_BF16, 3 * d, d);
            S.ref(blk_name(l, "qkv_c1"), Ly.qkv_c1, ST_F32, 3 * d); S.ref(blk_name(l, "qkv_b1"), Ly.qkv_b1, ST_F32, 3 * d);
        }
        S.ref(blk_name(l, "wup"), P.fold_ln3 ? Ly.up_wf : Ly.up_w, ST_BF16, hid, d);
        S.ref(blk_name(l, "up_c1"), Ly.up_c1, ST_F32, hid); S.ref(blk_name(l, "up_b1"), Ly.up_b1, ST_F32, hid);
        S.ref(blk_name(l, "wdown"), Ly.down_w, ST_BF16, d, hid);
        if (P.fp8) {   // the weights as held: e4m3 + E8M0, dequantised on read
            if (Stage* st = S.ref(blk_name(l, "wqkv"), Ly.qkv_w8, ST_MX8W, 3 * d, d)) st->aux = Ly.qkv_s8;
            if (Stage* st = S.ref(blk_name(l, "wup"), Ly.up_w8, ST_MX8W, hid, d)) st->aux = Ly.up_s8;
            if (Stage* st = S.ref(blk_name(l, "wdown"), Ly.down_w8, ST_MX8W, d, hid)) st->aux = Ly.down_s8;
        }
        // every other image of the block, in storage order (an image this mode does not hold -- a null pointer -- gets no name)
        for (const BodyImage& q : images)
            if (q.name) S.ref(blk_name(l, "img.") + q.name, q.get(Ly), q.dtype, q.shape[0], q.shape[1], q.shape[2], q.shape[3]);
    }
    {   // ... and of those outside the blocks
        StageStore& S = e->stages;
        const int64_t dd = e->d, ne = e->ne, pd = e->pd, K = e->d + e->hid;
        S.ref("img.angular", e->angular, ST_F32, ne / 2); S.ref("img.ff1_w", e->ff1_w, ST_F32, dd, ne); S.ref("img.ff1_b", e->ff1_b, ST_F32, dd);
        S.ref("img.ff3_w", e->ff3_w, ST_F32, dd, dd); S.ref("img.ff3_b", e->ff3_b, ST_F32, dd);
        S.ref("img.label_w", e->label_w, ST_F32, dd, e->text); S.ref("img.label_b", e->label_b, ST_F32, dd);
        S.ref("img.norm_w", e->norm_w, ST_F32, dd); S.ref("img.norm_b", e->norm_b, ST_F32, dd);
        S.ref("img.conv_w", e->conv_w, ST_F32, pd, pd); S.ref("img.conv_b", e->conv_b, ST_F32, pd);
        S.ref("img.pln1_w", e->pln1_w, ST_F32, pd); S.ref("img.pln1_b", e->pln1_b, ST_F32, pd); S.ref("img.plin_b", e->plin_b, ST_F32, dd);
        S.ref("img.pln2_w", e->pln2_w, ST_F32, dd); S.ref("img.pln2_b", e->pln2_b, ST_F32, dd); S.ref("img.pos", e->pos, ST_F32, e->ntok, dd);
        S.ref("img.out_w", e->out_w, ST_F32, pd, dd); S.ref("img.out_b", e->out_b, ST_F32, pd);
        S.ref("img.out_w_hl", e->out_w_hl, ST_BF16, 2, pd, dd); S.ref("img.plin_w_hl", e->plin_w_hl, ST_BF16, 2, dd, pd); S.ref("img.plin_wt", e->plin_wt, ST_F32, pd, dd);
        S.ref("img.out_fold_hl", e->mb.out_fold_hl, ST_BF16, 2, tail_fold_padded_rows(e->pd), K); S.ref("img.out_fold_b", e->mb.out_fold_b, ST_F32, pd);
    }
    return TLD_OK;
}

// start of a debug forward: what its kernels are to write holds NaN (0xFF bytes), so a kernel that stores nothing, or too few rows, shows
int debug_poison(tld_engine* e, hipStream_t s) {
    if (!e->debug) return TLD_OK;
    for (const auto& pb : e->poison) HIP_TRY(hipMemsetAsync(pb.first, 0xFF, pb.second, s));
    const size_t M = (size_t)e->cfg.max_batch * e->ntok;
    if (e->mb.splitk_slices) HIP_TRY(hipMemsetAsync(e->mb.splitk, 0xFF, (size_t)e->mb.splitk_slices * M * e->d * 4, s));
    if (e->mode.fp8) { HIP_TRY(hipMemsetAsync(e->a8, 0xFF, M * e->hid, s)); HIP_TRY(hipMemsetAsync(e->as8, 0xFF, M * e->hid / 32 + 1024, s)); }
    return TLD_OK;
}
// ... and of a debug call: the conditioning tables too; the launch-path record starts empty; the tables get their names for this call's T rows
int debug_begin(tld_engine* e, int T, int Tn, hipStream_t s) {
    if (!e->debug) return TLD_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(TLD_ERR_STATE, "a debug forward (tld_engine_set_debug) cannot be captured into a graph");
    e->paths = 0;
    const size_t cap = (size_t)e->cond_cap, d = e->d, L = e->L, H = e->H;
    for (float* p : {e->c_sin, e->c_h1, e->c_pre, e->c_y}) HIP_TRY(hipMemsetAsync(p, 0xFF, cap * (p == e->c_sin ? (size_t)e->ne : d) * 4, s));
    HIP_TRY(hipMemsetAsync(e->c_kv, 0xFF, L * cap * 2 * d * 4, s));
    HIP_TRY(hipMemsetAsync(e->c_wq, 0xFF, L * cap * H * d * 4, s));
    HIP_TRY(hipMemsetAsync(e->c_bwq, 0xFF, L * cap * H * 4, s));
    StageStore& S = e->stages;
    S.begin_call();      // every snapshot of an earlier call is forgotten (the operand names stay)
    S.ref("cond.sin", e->c_sin, ST_F32, Tn, e->ne); S.ref("cond.h1", e->c_h1, ST_F32, Tn, d);      // (noise rows only)
    S.ref("cond.pre", e->c_pre, ST_F32, T, d); S.ref("cond.y", e->c_y, ST_F32, T, d);
    S.ref("cond.kv", e->c_kv, ST_F32, L, T, 2 * d, 1, (int64_t)(cap * 2 * d));
    S.ref("cond.wq", e->c_wq, ST_F32, L, T, H, d, (int64_t)(cap * H * d));
    S.ref("cond.bwq", e->c_bwq, ST_F32, L, T, H, 1, (int64_t)(cap * H));
    return TLD_OK;
}
struct PathScope {      // the launchers record their paths into this engine while one of its debug calls runs on this thread; no stage is kept after it, on any exit
    tld_engine* e;
    explicit PathScope(tld_engine* e_) : e(e_) { if (e->debug) g_path_sink = &e->paths; }
    ~PathScope() { g_path_sink = nullptr; e->dbg_keep = false; }
};

// Conditioning tables for T token rows whose pre-LN vectors sit in c_pre[0..T): y = LN(pre), then per
// layer K|V = y Wkv^T and the folded query vectors (denoiser.py:121-122, transformer_blocks.py:65-71).
int cond_tables(tld_engine* e, int T, hipStream_t s) {
    const int d = e->d;
    ProfScope ps(e, KC_COND, s);
    launch_layernorm_f32(e->c_pre, e->norm_w, e->norm_b, e->c_y, T, d, s);
    // all layers in two launches (blockIdx.z = layer; per-layer weights through pointer tables): these are small
    // fp32 problems (T ~ 100 token rows), 24 dependent launches of them were 2 ms per generate
    launch_linear_f32_layers(e->c_y, d, e->tab_kv_w, e->c_kv, (size_t)e->cond_cap * 2 * d, 2 * d, T, d, 2 * d, e->L, s);
    launch_wq_layers(e->c_kv, (size_t)e->cond_cap * 2 * d, 2 * d, e->tab_q_w, e->tab_n2_w, e->tab_n2_b, e->c_wq,
                     (size_t)e->cond_cap * e->H * d, e->c_bwq, (size_t)e->cond_cap * e->H, T, e->H, d, e->L, s);
    return TLD_OK;
}

// noise rows: sigma[0..Tn) in c_sigma -> c_pre[0..Tn)   (denoiser.py:105-110,117)
void cond_noise_rows(tld_engine* e, int Tn, hipStream_t s) {
    launch_sinusoid(e->c_sigma, e->angular, e->c_sin, Tn, e->ne / 2, s);
    launch_linear_f32(e->c_sin, e->ne, e->ff1_w, e->ff1_b, e->c_h1, e->d, Tn, e->ne, e->d, 1, s);
    launch_linear_f32(e->c_h1, e->d, e->ff3_w, e->ff3_b, e->c_pre, e->d, Tn, e->d, e->d, 0, s);
}

// label rows: c_label[0..Tl) -> c_pre[row0 .. row0+Tl)   (denoiser.py:114,119)
void cond_label_rows(tld_engine* e, int row0, int Tl, hipStream_t s) {
    launch_linear_f32(e->c_label, e->text, e->label_w, e->label_b, e->c_pre + (size_t)row0 * e->d, e->d, Tl,
                      e->text, e->d, 0, s);
}

// embed -> L decoder blocks -> tail, for `batch` model samples whose latents are x_src[b % src_batch], or x_src[src_row[b]] with a device table
// src_row [batch] whose first src_batch entries are the identity (src_batch <= batch <= 2 src_batch: the unconditional samples are a subset).
// share_l0: the model batch is [x_src ; x_src] (CFG doubling), so everything before the first cross-attention --
// patch embedding, LN1, the QKV GEMM and self-attention of block 0 -- is identical for both halves and is
// computed for src_batch samples only; block 0's row kernel then fans it out to the 2*src_batch streams.
// embed_slot (a session step): a device table [batch] for the embed alone -- compact model sample k reads the latent x_src[embed_slot[k]], the
// slot of its request in the session's slot-major x_t; shared, the embed takes the first src_batch entries.  The fan-out keeps the compact src_row.
int run_body(tld_engine* e, const float* x_src, int src_batch, int batch, const int* noise_row,
             const int* label_row, float* out, hipStream_t s, bool share_l0 = false, const int* src_row = nullptr, const int* embed_slot = nullptr) {
    const int d = e->d, M = batch * e->ntok;
    share_l0 = share_l0 && e->mode.share_l0 && (src_row ? batch > src_batch && batch <= 2 * src_batch : batch == 2 * src_batch);
    if (int rc = debug_poison(e, s)) return rc;
    const int b0 = share_l0 ? src_batch : batch;            // samples processed up to block 0's attention
    resid_t* xe = share_l0 ? e->x_half : e->x;
    const BodyPlan& P = e->mode;                             // which path every stage below takes: decided once (tld_body_plan.h), read here
    const bool fold1 = P.fold_ln1;                           // LayerNorm-1 applied inside the QKV GEMM's epilogue
    const int ln_slots = gemm_resid_stat_slots(d);
    {
        ProfScope ps(e, KC_EMBED, s);
        EmbedParams ep{};
        ep.x = x_src; ep.conv_w = e->conv_w; ep.conv_b = e->conv_b; ep.ln1_w = e->pln1_w; ep.ln1_b = e->pln1_b;
        ep.lin_wt = e->plin_wt; ep.lin_w_hl = e->plin_w_hl; ep.lin_b = e->plin_b; ep.ln2_w = e->pln2_w; ep.ln2_b = e->pln2_b; ep.pos = e->pos;
        ep.tok = xe; ep.stats_out = fold1 ? e->ln_stats : nullptr; ep.batch = b0; ep.src_batch = src_batch; ep.C = e->cfg.n_channels;
        ep.src_row = embed_slot ? embed_slot : share_l0 ? nullptr : src_row;      // (shared: the first src_batch samples are the identity)
        ep.S = e->cfg.image_size; ep.p = e->cfg.patch_size; ep.grid = e->grid; ep.pd = e->pd; ep.d = d;
        ep.ntok = e->ntok;
        launch_embed(ep, s);
    }
    const int rdt = sizeof(resid_t) == 2 ? ST_BF16 : ST_F32;
    SNAP("tokens0", xe, rdt, s, (int64_t)b0 * e->ntok, d);
    for (int l = 0; l < e->L; ++l) {
        const Layer& Ly = e->layers[l];
        const bool half = share_l0 && l == 0;
        const int bl = half ? b0 : batch, Ml = bl * e->ntok;
        SNAP(blk_name(l, "x_in"), half ? xe : e->x, rdt, s, Ml, d);
        if (fold1) SNAP(blk_name(l, "ln1"), e->ln_stats, ST_F32, s, Ml, kLnSlots, 2);
        if (!fold1) {   // xn = LN1(x)
            ProfScope ps(e, KC_LN, s);
            if (P.ln_mx8) launch_layernorm_mx8(half ? xe : e->x, Ly.n1_w, Ly.n1_b, e->a8, e->as8, Ml, d, s);
            else { launch_layernorm_bf16(half ? xe : e->x, Ly.n1_w, Ly.n1_b, e->xn, Ml, d, s); SNAP(blk_name(l, "xn1"), e->xn, ST_BF16, s, Ml, d); }
        }
        // 256-token grids with the LayerNorm-1 fold: the QKV projection and the whole self-attention of a (sample, head) are one 256 x 192
        // GEMM tile + epilogue; q, k, v never reach HBM and `att` is written directly.  (the fp8 mode keeps the two kernels)
        const bool fused_qa = P.fused_qa;
        if (fused_qa) {
            ProfScope ps(e, KC_GEMM_QKV, s);
            GemmParams g{};
            const bool pair = body_pair_launch(P, bl);      // two heads per tile where that is the faster cut of this launch (the same bits either way)
            g.A = half ? xe : e->x; g.lda = d; g.W = pair ? Ly.qkv_wp2 : Ly.qkv_wp; g.ldw = d; g.M = Ml; g.N = 3 * d; g.K = d;
            g.out_bf16 = e->att; g.ldo = d; g.ntok = e->ntok; g.d = d;
            g.ln_stats = e->ln_stats; g.ln_slots = l == 0 ? 2 : ln_slots; g.ln_c1 = pair ? Ly.qkv_c1p2 : Ly.qkv_c1p; g.ln_b1 = pair ? Ly.qkv_b1p2 : Ly.qkv_b1p;
            g.park = pair ? e->mb.pair_park : nullptr;
            GEMM_TRY(blk_name(l, "QKV + attention"), launch_gemm(g, pair ? EPI_QKV_ATTN2 : EPI_QKV_ATTN, s));
        } else {   // q|k, v^T = LN1(x) Wqkv^T
            ProfScope ps(e, KC_GEMM_QKV, s);
            GemmParams g{};
            g.A = e->xn; g.lda = d; g.W = Ly.qkv_w; g.ldw = d; g.M = Ml; g.N = 3 * d; g.K = d;
            g.out_bf16 = e->qk; g.ldo = 2 * d; g.vt = e->vt; g.ntok = e->ntok; g.d = d;
            if (P.fp8) {   // MX-fp8: quantise LN1(x) (one pass over [M, d]; fused into the LayerNorm kernel when possible), then the e4m3 GEMM
                if (P.quant_qkv) launch_quant_mx8(e->xn, e->a8, e->as8, Ml, d, s);
                SNAP(blk_name(l, "a8_qkv.q"), e->a8, ST_U8, s, Ml, d); SNAP(blk_name(l, "a8_qkv.s"), e->as8, ST_MX8S, s, Ml, d / 32);
                g.f8 = 1; g.A = reinterpret_cast<const bf16*>(e->a8); g.W = reinterpret_cast<const bf16*>(Ly.qkv_w8);
                g.a_scale = e->as8; g.w_scale = Ly.qkv_s8;
            }
#ifdef TLD_RESID_BF16
            if (fold1) {    // raw residual rows x gamma-scaled weights; partial sums from embed (block 0) / the down projection
                g.A = half ? xe : e->x; g.W = Ly.qkv_wf; g.ln_stats = e->ln_stats; g.ln_slots = l == 0 ? 2 : ln_slots;
                g.ln_c1 = Ly.qkv_c1; g.ln_b1 = Ly.qkv_b1;
            }
#endif
            GEMM_TRY(blk_name(l, "QKV projection"), launch_gemm(g, fold1 ? EPI_QKV_LN : EPI_QKV, s));
            SNAP(blk_name(l, "qk"), e->qk, ST_BF16, s, Ml, 2 * d); SNAP(blk_name(l, "vt"), e->vt, ST_BF16, s, bl, d, e->ntok);
        }
        if (!fused_qa) {
            ProfScope ps(e, KC_ATTN, s);
            launch_attention(e->qk, e->vt, e->att, bl, e->ntok, e->H, s);
        }
        SNAP(blk_name(l, "att"), e->att, ST_BF16, s, Ml, d);
        // 256 px (16x16 tokens): one GEMM tile row-block is one image, so the depthwise conv + GELU run inside the
        // up-projection's epilogue and the pre-conv hidden never reaches HBM.  Other grids: separate kernels.
        // 512 px (32x32 tokens, round 4): a tile row-block is 8 image rows; the epilogue finishes the interior rows and a thin second kernel the two rows at
        // every tile seam from the hidden rows the epilogue leaves for it (half of the hidden tensor instead of a write + read of all of it).
        const bool fuse_dw = P.fuse_dw;
        const bool fold3 = P.fold_ln3;                  // LN3 applied in the up-projection's epilogue: cross_row writes row statistics, not xn
        {   // x += att; x += CA(LN2 x, y); xn = LN3(x) (or its row statistics)
            ProfScope ps(e, KC_CROSS, s);
            CrossRowParams cp{};
            cp.x = e->x; cp.att = e->att;
            cp.x_in = half ? xe : nullptr; cp.src_batch = src_batch; cp.src_row = src_row;
            cp.wq = e->c_wq + (size_t)l * e->cond_cap * e->H * d;
            cp.bwq = e->c_bwq + (size_t)l * e->cond_cap * e->H;
            cp.v = e->c_kv + (size_t)l * e->cond_cap * 2 * d + d;     // V half of each [2d] row
            cp.v_ld = 2 * d;
            cp.noise_row = noise_row; cp.label_row = label_row;
            cp.ln2_w = Ly.n2_w; cp.ln2_b = Ly.n2_b; cp.ln3_w = Ly.n3_w; cp.ln3_b = Ly.n3_b;
            cp.xn3 = fold3 ? nullptr : e->xn; cp.ln3_stats = fold3 ? e->row_stats : nullptr; cp.batch = batch; cp.ntok = e->ntok; cp.d = d; cp.heads = e->H;
            if (e->dbg_keep) { if (int rc = e->stages.sink(blk_name(l, "sa"), M, d, &cp.sa_out)) return rc; }
            const bool cross8 = P.cross_mx8;
            if (cross8) { cp.xn3_f8 = e->a8; cp.xn3_s8 = e->as8; }
            launch_cross_row(cp, s);
            if (!fold3 && !cross8) SNAP(blk_name(l, "xn3"), e->xn, ST_BF16, s, M, d);
        }
        SNAP(blk_name(l, "ca"), e->x, rdt, s, M, d);
        if (fold3) SNAP(blk_name(l, "stats"), e->row_stats, ST_F32, s, M, 2);
        if (fuse_dw) {
            ProfScope ps(e, KC_GEMM_UP, s);
            GemmParams g{};
            g.A = e->xn; g.lda = d; g.W = Ly.up_w; g.ldw = d; g.M = M; g.N = e->hid; g.K = d;
            g.out_bf16 = e->hid2; g.ldo = e->hid; g.bias = Ly.up_b; g.dw_b = Ly.dw_b_half;
            g.dw_wpk = Ly.dw_wpk;
#ifdef TLD_RESID_BF16
            if (fold3) {    // LN3 inside the epilogue: raw residual rows x gamma-scaled weights, statistics from cross_row
                g.A = e->x; g.W = Ly.up_wf; g.bias = Ly.up_b1; g.ln_c1 = Ly.up_c1; g.row_stats = e->row_stats;
            }
#endif
            g.dw_seam = e->mb.seam;
            GEMM_TRY(blk_name(l, "fused up-projection"), launch_gemm(g, P.seam ? EPI_UP_DWCONV32 : EPI_UP_DWCONV2, s));
            if (P.seam) {
                ProfScope ps2(e, KC_DWCONV, s);
                launch_dwconv_seam(e->mb.seam, Ly.dw_wpk, Ly.dw_b_half, e->hid2, e->hid, batch, e->hid, s);
            }
        } else {
            {   // hid1 = xn Wup^T + b
                ProfScope ps(e, KC_GEMM_UP, s);
                GemmParams g{};
                g.A = e->xn; g.lda = d; g.W = Ly.up_w; g.ldw = d; g.M = M; g.N = e->hid; g.K = d;
                g.out_bf16 = e->hid1; g.ldo = e->hid; g.bias = Ly.up_b;
                if (P.fp8) {
                    if (P.quant_up) launch_quant_mx8(e->xn, e->a8, e->as8, M, d, s);
                    SNAP(blk_name(l, "a8_up.q"), e->a8, ST_U8, s, M, d); SNAP(blk_name(l, "a8_up.s"), e->as8, ST_MX8S, s, M, d / 32);
                    g.f8 = 1; g.A = reinterpret_cast<const bf16*>(e->a8); g.W = reinterpret_cast<const bf16*>(Ly.up_w8);
                    g.a_scale = e->as8; g.w_scale = Ly.up_s8;
                }
#ifdef TLD_RESID_BF16
                if (fold3) {
                    g.A = e->x; g.W = Ly.up_wf; g.bias = Ly.up_b1; g.ln_c1 = Ly.up_c1; g.row_stats = e->row_stats;
                }
#endif
                GEMM_TRY(blk_name(l, "up-projection"), launch_gemm(g, EPI_BIAS_BF16, s));
            }
            SNAP(blk_name(l, "hid_pre"), e->hid1, ST_BF16, s, M, e->hid);
            {
                ProfScope ps(e, KC_DWCONV, s);
                const bool dw8 = P.dw_mx8;                    // the tiled kernel writes the fp8 operand of the down projection itself
                launch_dwconv_gelu(e->hid1, e->hid2, Ly.dw_w9c, Ly.dw_b, Ly.dw_w9c_half, Ly.dw_b_half, batch, e->grid, e->hid, s,
                                   dw8 ? e->a8 : nullptr, dw8 ? e->as8 : nullptr);
            }
        }
        if (!P.dw_mx8) SNAP(blk_name(l, "hid"), e->hid2, ST_BF16, s, M, e->hid);      // (the quantising depthwise kernels write no bf16 copy)
        // The last block, default class, bf16 operands: its down projection is folded into out_proj.  The 768-wide row
        // x3 = x2 + hid2 Wd^T + bd is read by out_proj alone, so the tail below takes [x2 | hid2] against [Wout | Wout Wd] and the GEMM is not launched.
        const bool fold_tail = l + 1 == e->L && P.fold_tail;
#ifdef TLD_RESID_BF16
        if (fold_tail && e->dbg_keep) {
            // stage hook only: the row the folded tail stands for, unrounded, as an fp32 stage in the hook's own memory (like cross_row's sa dump: no
            // product buffer is touched and no launch path is recorded) -- hid2 Wd^T by the fp32-output GEMM, then x2 and the bias per element
            float* row = nullptr;
            if (int rc = e->stages.sink(blk_name(l, "mlp"), M, d, &row)) return rc;
            GemmParams g{};
            g.A = e->hid2; g.lda = e->hid; g.W = Ly.down_w; g.ldw = e->hid; g.M = M; g.N = d; g.K = e->hid; g.c_f32 = row; g.ldc = d;
            uint64_t* const sink = g_path_sink;
            g_path_sink = nullptr;
            const int rc = launch_gemm(g, EPI_F32, s);
            g_path_sink = sink;
            if (rc) { const std::string m = tld_last_error(); return fail(rc, "%s (debug row of the folded tail): %s", blk_name(l, "mlp").c_str(), m.c_str()); }
            launch_tail_fold_debug_row(row, e->x, Ly.down_b, M, d, s);
        }
#endif
        if (fold_tail) {
            // (nothing here: launch_tail after the loop)
        } else if (P.ll_split) {
            // Low-latency class: a handful of samples are a handful of 256-row tiles, and the down projection's 48 K-steps per tile (K = 4 d) were
            // half of a layer's time however empty the chip was.  Four K-splits quadruple the work items (fp32 slices, summed in a fixed order by
            // the finishing kernel together with bias, residual add and the LayerNorm-1 partial sums).  Results differ from the default class in the
            // fp32 summation order of that one product -- which is why the class is a property of the ENGINE (chosen by the caller, checked against
            // its capacity), never of the batch a call happens to carry: inside a class results stay bit-identical across batch sizes.
            ProfScope ps(e, KC_GEMM_DOWN, s);
            GemmParams g{};
            g.A = e->hid2; g.lda = e->hid; g.W = Ly.down_w; g.ldw = e->hid; g.M = M; g.N = d; g.K = e->hid / P.ll_split; g.ksplit = P.ll_split;
            g.c_f32 = e->mb.splitk; g.ldc = d;
            GEMM_TRY(blk_name(l, "split-K down projection"), launch_gemm(g, EPI_F32, s));
            SNAP(blk_name(l, "splitk"), e->mb.splitk, ST_F32, s, P.ll_split, M, d);
            launch_splitk_resid(e->mb.splitk, P.ll_split, (size_t)M * d, Ly.down_b, e->x, (fold1 && l + 1 < e->L) ? e->ln_stats : nullptr, M, d, s);
        } else
        {   // x += hid2 Wdown^T + b
            ProfScope ps(e, KC_GEMM_DOWN, s);
            GemmParams g{};
            g.A = e->hid2; g.lda = e->hid; g.W = Ly.down_w; g.ldw = e->hid; g.M = M; g.N = d; g.K = e->hid;
            g.bias = Ly.down_b; g.resid = e->x; g.ldr = d;
            g.stats_out = (fold1 && l + 1 < e->L) ? e->ln_stats : nullptr;
            if (P.fp8) {
                if (P.quant_down) launch_quant_mx8(e->hid2, e->a8, e->as8, M, e->hid, s);
                SNAP(blk_name(l, "a8_down.q"), e->a8, ST_U8, s, M, e->hid); SNAP(blk_name(l, "a8_down.s"), e->as8, ST_MX8S, s, M, e->hid / 32);
                g.f8 = 1; g.A = reinterpret_cast<const bf16*>(e->a8); g.W = reinterpret_cast<const bf16*>(Ly.down_w8);
                g.a_scale = e->as8; g.w_scale = Ly.down_s8;
            }
            GEMM_TRY(blk_name(l, "down projection"), launch_gemm(g, EPI_BIAS_RESID, s));
        }
        if (!fold_tail) SNAP(blk_name(l, "mlp"), e->x, rdt, s, M, d);
    }
    {
        ProfScope ps(e, KC_TAIL, s);
        TailParams tp{};
        tp.tok = e->x; tp.w = e->out_w; tp.w_hl = e->out_w_hl; tp.b = e->out_b; tp.out = out; tp.batch = batch;
        tp.C = e->cfg.n_channels; tp.S = e->cfg.image_size; tp.p = e->cfg.patch_size; tp.grid = e->grid;
        tp.pd = e->pd; tp.d = d; tp.ntok = e->ntok;
        if (P.fold_tail) {      // (the last block's down projection was not launched: e->x is x2, the row before it)
            tp.hid = e->hid2; tp.hidn = e->hid; tp.wf_hl = e->mb.out_fold_hl; tp.bf = e->mb.out_fold_b;
        }
        launch_tail(tp, s);
    }
    SNAP("out", out, ST_F32, s, batch, e->img);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

// The device side of a sampler call, beside its SampleCall (tld_sample_plan.h)
struct SampleOperands {
    const float *noise, *init_latent, *mask, *labels, *neg_labels;      // init_latent / mask / neg_labels optional
    float sharp, bright;
    float *out_latent, *trace_x0, *trace_xt;
    int path_step, path_start;           // the EP_UPDATE* / EP_START_MIX* bits of the calling entry
    bool keep_stages;                    // step.* and the body's stages are kept at the debug step (the uniform entries)
};

// The one sampler loop: conditioning tables of every request's whole trajectory, the start, then per step of the plan the model on the requests that
// still run (a shrinking prefix, CFG-doubled, layer-0 sharing) and the elementwise step.  Host-built tables travel through the engine's pinned staging
// buffer in two uploads behind stage_ev: no stream synchronisation.  Conditioning rows: Tn noise rows, B label rows, the zero row, one row per negative label.
// In the slots flavour the model batch of step i is [Bi conditional | U_i unconditional] samples, U_i the requests guided at that step: the step's
// rows then carry a third table, the request each model sample reads, and a request's step row its unconditional slot.
int run_sampler(tld_engine* e, const SamplePlan& plan, const SampleCall& call, const SampleOperands& p, hipStream_t s) {
    const int B = plan.B, n_max = plan.n_max, Tn = plan.Tn, T = plan.T, tabB = plan.tabB;
    const bool any_mom = plan.any_mom;
    if (int rc = ensure_cond_capacity(e, T)) return rc;
    if (int rc = ensure_req_capacity(e, plan.up_bytes)) return rc;
    if (plan.any_shape && !e->shape_pq)
        if (int rc = dev_alloc(e, &e->shape_pq, (size_t)e->cfg.max_batch)) return rc;
    if (plan.any_shape && !e->shape_sums)
        if (int rc = dev_alloc(e, &e->shape_sums, (size_t)e->cfg.max_batch * GS_SUMS)) return rc;
    if (any_mom && !e->shape_mom)
        if (int rc = dev_alloc(e, &e->shape_mom, (size_t)e->cfg.max_batch * e->img)) return rc;
    if (int rc = debug_begin(e, T, Tn, s)) return rc;
    if (int rc = stage_acquire(e, plan.stage_bytes)) return rc;
    sample_plan_fill(plan, call, e->stage_host);
    e->rows_cond = plan.rows_cond; e->rows_uncond = plan.rows_uncond;
    const float* sigs = reinterpret_cast<const float*>(static_cast<const char*>(e->stage_host) + plan.up_bytes);
    const int n_neg = plan.n_neg;

    // ---- conditioning tables for every request's whole trajectory, once
    const size_t text = e->text;
    HIP_TRY(hipMemcpyAsync(e->c_sigma, sigs, (size_t)Tn * sizeof(float), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(e->c_label, p.labels, (size_t)B * text * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(e->c_label + (size_t)B * text, 0, text * sizeof(float), s));     // uncond = zeros (diffusion.py:61)
    for (int b = 0, k = 0; b < B && n_neg; ) {                // negative labels, compacted: one copy per run of consecutive requests that have one
        if (!call.req(b).has_negative) { ++b; continue; }
        int b1 = b;
        while (b1 < B && call.req(b1).has_negative) ++b1;
        HIP_TRY(hipMemcpyAsync(e->c_label + (size_t)(B + 1 + k) * text, p.neg_labels + (size_t)b * text, (size_t)(b1 - b) * text * sizeof(float),
                               hipMemcpyDeviceToDevice, s));
        k += b1 - b; b = b1;
    }
    {
        ProfScope ps(e, KC_COND, s);
        cond_noise_rows(e, Tn, s);
        cond_label_rows(e, Tn, B + 1 + n_neg, s);
    }
    if (int rc = cond_tables(e, T, s)) return rc;
    HIP_TRY(hipMemcpyAsync(e->req_dev, e->stage_host, plan.up_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(e->stage_ev, s));     // no stream sync: the staging buffer is the engine's, guarded by this event
    const char* dev = static_cast<const char*>(e->req_dev);
    const SamplerStepRow* tab_dev = reinterpret_cast<const SamplerStepRow*>(dev);
    const float* mix_dev = reinterpret_cast<const float*>(dev + plan.mix_off);
    const int* rows_dev = reinterpret_cast<const int*>(dev + plan.rows_off);
    const SamplerNoiseRow* noise_dev = plan.noise ? reinterpret_cast<const SamplerNoiseRow*>(dev + plan.noise_off) : nullptr;
    const GuidanceShape* shape_dev = plan.shape ? reinterpret_cast<const GuidanceShape*>(dev + plan.shape_off) : nullptr;

    // ---- the start: pure noise at the schedule's first level (diffusion.py:52,59), else the forward process at the first remaining level (train.py:130)
    const size_t tot = (size_t)B * e->img;
    if (!plan.any_mix) HIP_TRY(hipMemcpyAsync(e->xt, p.noise, tot * sizeof(float), hipMemcpyDeviceToDevice, s));
    else launch_start_mix(p.noise, p.init_latent, mix_dev, plan.stride, e->xt, B, e->img, p.path_start, s);
    HIP_TRY(hipMemsetAsync(e->x0_prev, 0, tot * sizeof(float), s));
    if (any_mom) HIP_TRY(hipMemsetAsync(e->shape_mom, 0, tot * sizeof(float), s));      // the momentum starts every call at zero
    // ---- the steps over the shrinking prefix of requests that still run
    for (int i = 0; i < n_max; ++i) {
        const SampleStep& st = plan.steps[(size_t)i];
        const bool last = i == n_max - 1;
        const int Bi = st.Bi, mb = st.mb;
        const int* nr = rows_dev + st.rows_off;
        // At the debug step (tld_engine_set_debug_step; every step when it is negative) the body's stages are kept, and so are the step's inputs
        // (x_t, x0_prev) and outputs (the 2B forward output, the x0 written, the next x_t).
        if (p.keep_stages) e->dbg_keep = e->debug && (e->dbg_step < 0 || e->dbg_step == i);
        SNAP("step.x_t", e->xt, ST_F32, s, B, e->img); SNAP("step.x0_prev", e->x0_prev, ST_F32, s, B, e->img);
        // pred_image: model(cat[x_t, x_t], sigma_i, [labels; 0])   (diffusion.py:94-101)
        if (int rc = run_body(e, e->xt, Bi, mb, nr, nr + mb, e->io_out, s, true, plan.slots ? nr + 2 * mb : nullptr)) return rc;
        SamplerStepParams up{};
        up.x0_2b = e->io_out; up.x_t = e->xt; up.x0_prev = e->x0_prev; up.out_latent = p.out_latent;
        up.trace_x0 = (!last && p.trace_x0) ? p.trace_x0 + (size_t)i * tot : nullptr;
        up.trace_xt = (!last && p.trace_xt) ? p.trace_xt + (size_t)i * tot : nullptr;
        up.noise = p.noise; up.z0 = p.init_latent; up.mask = p.mask;
        up.rows = tab_dev + (size_t)i * tabB; up.row_stride = plan.stride; up.sharp = p.sharp; up.bright = p.bright;
        up.active = Bi; up.img = e->img; up.chan_stride = e->cfg.image_size * e->cfg.image_size;
        if (plan.noise) { up.noise_rows = noise_dev + (size_t)i * tabB; up.noise_step = (uint32_t)i; }
        // a step at which no running request is shaped and guided needs neither the statistics nor the SHAPE flavour: it would take `combine` for every
        // request, which the NOISE flavour does with one table less to read
        if (st.stats) {       // (P, Q) of the requests shaped at this step, before the step reads them
            up.shape_rows = shape_dev; up.shape_pq = e->shape_pq; up.shape_mom = any_mom ? e->shape_mom : nullptr;
            GuidanceStatsParams gp{};
            gp.cond = e->io_out; gp.unc_base = e->io_out + (size_t)Bi * e->img; gp.mom = up.shape_mom; gp.rows = up.rows; gp.shape_rows = shape_dev;
            gp.row_stride = plan.stride; gp.active = Bi; gp.img = e->img; gp.pq = e->shape_pq; gp.sums = e->shape_sums;
            ProfScope ps(e, KC_UPDATE, s);
            launch_guidance_stats(gp, s);
        }
        {
            ProfScope ps(e, KC_UPDATE, s);
            launch_sampler_step(up, p.path_step, s, plan.slots);
        }
        // (the uniform entries: every sample is at its last level together, and an inner step has just stored its prediction to x0_prev)
        SNAP("step.out", e->io_out, ST_F32, s, 2 * B, e->img); SNAP("step.x0", last ? p.out_latent : e->x0_prev, ST_F32, s, B, e->img);
        if (!last) SNAP("step.x_next", e->xt, ST_F32, s, B, e->img);
        e->dbg_keep = false;
    }
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

// Every sampler entry: check, the engine's state, plan, run.  The uniform entries have tested their pointers before the checks, the others test them here.
int sample_requests(tld_engine* e, SampleCall& call, const SampleOperands& ops, void* hip_stream) {
    // the records first: their checks need no engine and no device
    if (SampleRefusal r = sample_call_check(call)) return fail(r.code, "%s", r.msg.c_str());
    if (!e || !ops.noise || !ops.labels || !ops.out_latent) return fail(TLD_ERR_INVALID, "null argument");
    if (!e->finalized) return fail(TLD_ERR_STATE, "weights not finalized");
    if (e->session) return fail(TLD_ERR_STATE, "a sampler session is open on this engine: it owns the conditioning tables and the sampler buffers (tld_session_close first)");
    call.guidance_skip = e->mode.guidance_skip; call.max_batch = e->cfg.max_batch;
    if (SampleRefusal r = sample_plan(call, e->plan)) return fail(r.code, "%s", r.msg.c_str());
    DeviceGuard dg(e->cfg.device_id);
    PathScope paths(e);                                       // (debug: the launch paths are recorded; the requests entries keep no stage)
    return run_sampler(e, e->plan, call, ops, static_cast<hipStream_t>(hip_stream));
}

SampleOperands sample_operands(const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels, float sharp_f,
                               float bright_f, void* out_latent, void* trace_x0, void* trace_xt, int path_step, int path_start, bool keep_stages) {
    return SampleOperands{static_cast<const float*>(noise), static_cast<const float*>(init_latent), static_cast<const float*>(mask),
                          static_cast<const float*>(labels), static_cast<const float*>(neg_labels), sharp_f, bright_f, static_cast<float*>(out_latent),
                          static_cast<float*>(trace_x0), static_cast<float*>(trace_xt), path_step, path_start, keep_stages};
}

// tld_sample / tld_sample_from after their pointer tests: one record and one coefficient table for the whole batch; noise row i is level i
int run_uniform(tld_engine* e, const void* noise, const void* init_latent, const void* mask, float start_mix, const void* labels, const float* coeffs,
                int n_levels, float class_guidance, float sharp_f, float bright_f, void* out_latent, int batch, void* trace_x0, void* trace_xt,
                int path_step, void* hip_stream) {
    const tld_sample_request rec{n_levels, class_guidance, start_mix, 0};
    SampleCall call{};
    call.entry = SE_UNIFORM; call.B = batch; call.n_max = n_levels; call.stride = 0; call.requests = &rec; call.coeffs = coeffs;
    call.has_mask = mask != nullptr; call.has_init = init_latent != nullptr;
    SampleOperands ops = sample_operands(noise, init_latent, mask, labels, nullptr, sharp_f, bright_f, out_latent, trace_x0, trace_xt, path_step, EP_START_MIX, true);
    return sample_requests(e, call, ops, hip_stream);
}

// the four tld_sample_requests* entries: a record and a coefficient table per request; guidance, noise_coeff + noise_keys and shape as the entry has them
int run_requests(SampleEntry entry, tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
                 const tld_sample_request* requests, const float* coeffs, const float* guidance, const float* noise_coeff, const uint64_t* noise_keys,
                 const float* shape, int n_max, float sharp_f, float bright_f, void* out_latent, int batch, void* trace_x0, void* trace_xt, void* hip_stream) {
    SampleCall call{};
    call.entry = entry; call.B = batch; call.n_max = n_max; call.stride = 1; call.requests = requests; call.coeffs = coeffs;
    call.guidance = guidance; call.noise_coeff = noise_coeff; call.noise_keys = noise_keys; call.shape = shape;
    call.has_mask = mask != nullptr; call.has_init = init_latent != nullptr; call.has_neg_labels = neg_labels != nullptr;
    SampleOperands ops = sample_operands(noise, init_latent, mask, labels, neg_labels, sharp_f, bright_f, out_latent, trace_x0, trace_xt,
                                         mask ? EP_UPDATE_REQ_MASK : EP_UPDATE_REQ, EP_START_MIX_REQ, false);
    return sample_requests(e, call, ops, hip_stream);
}

}  // namespace

// ================================================================================================
extern "C" {

const char* tld_last_error(void) { return g_err; }


int tld_engine_create(const tld_config* c, tld_engine** out) {
    if (!c || !out) return fail(TLD_ERR_INVALID, "null argument");
    *out = nullptr;
    // (the runtime is asked for the device count only once the configuration has passed every refusal in front of the device_id one)
    if (const std::string bad = body_config_check(*c, -1); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (const std::string bad = body_config_check(*c, ndev); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    DeviceGuard dg(c->device_id);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c->device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(TLD_ERR_INVALID, "device %d is %s; this engine is built for gfx950 only", c->device_id, prop.gcnArchName);
    tld_engine* e = new tld_engine();
    e->cfg = *c;
    static_cast<BodyShape&>(*e) = body_shape(*c);
    e->layers.resize(e->L);
    e->nparam = make_param_layout(e->d, e->L, e->ne, e->pd, e->hid, e->ntok, e->text).count;
    e->sw = body_switches(getenv);
    replan(e, false, 0);
    *out = e;
    return TLD_OK;
}

int tld_engine_load_tensor(tld_engine* e, const char* key, const void* host_ptr, const int64_t* shape,
                           int32_t ndim, int32_t dtype) {
    if (!e || !key || (!host_ptr && ndim > 0)) return fail(TLD_ERR_INVALID, "null argument");
    if (e->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    if (strstr(key, "precomputed_pos_enc")) return TLD_OK;          // arange buffer (denoiser.py:55)
    if (dtype != TLD_DTYPE_F32) return fail(TLD_ERR_INVALID, "%s: only fp32 state_dict tensors are accepted", key);
    int64_t n = 1;
    HostTensor t;
    for (int i = 0; i < ndim; ++i) { n *= shape[i]; t.shape.push_back(shape[i]); }
    t.data.assign(static_cast<const float*>(host_ptr), static_cast<const float*>(host_ptr) + n);
    e->host[key] = std::move(t);
    return TLD_OK;
}

// Allocates every weight image this engine's mode holds, uploads the loaded fp32 tensors as ONE temporary flat vector in ParamLayout order and lets the
// refresh kernels (tld_refresh.hip: the one builder of every image) fill them; then the activation buffers.  No arithmetic on weight values happens here.
int tld_engine_finalize_weights(tld_engine* e) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    if (e->finalized) return TLD_OK;
    DeviceGuard dg(e->cfg.device_id);
    const int64_t d = e->d, ne = e->ne, pd = e->pd, hid = e->hid, N = e->ntok, text = e->text;
    const ParamLayout pl = make_param_layout(e->d, e->L, e->ne, e->pd, e->hid, e->ntok, e->text);
    // the loaded state dict: every parameter present, with its element count (keys outside the layout are ignored)
    const auto loaded = [e](const std::string& key, int64_t numel, const HostTensor** out) -> int {
        auto it = e->host.find(key);
        if (it == e->host.end()) return fail(TLD_ERR_STATE, "state_dict entry missing: %s", key.c_str());
        if ((int64_t)it->second.data.size() != numel)
            return fail(TLD_ERR_SHAPE, "%s: expected %lld elements, got %lld", key.c_str(), (long long)numel, (long long)it->second.data.size());
        *out = &it->second;
        return TLD_OK;
    };
    const HostTensor* t = nullptr;
    for (const ParamTensor& q : pl.tensors) if (int rc = loaded(q.key, q.numel, &t)) return rc;
    if (int rc = loaded("fourier_feats.0.angular_speeds", ne / 2, &t)) return rc;      // a buffer, not a parameter: not in the flat vector
#define IMG(ptr, n) if (int rc = dev_alloc(e, &(ptr), (size_t)(n), true)) return rc;
    IMG(e->angular, ne / 2)
    HIP_TRY(hipMemcpy(e->angular, t->data.data(), (size_t)(ne / 2) * sizeof(float), hipMemcpyHostToDevice));
    // the images outside the blocks, each with its place in the flat vector
    RefreshPlan& R = e->refresh;
    R = RefreshPlan();
    R.d = e->d; R.hid = e->hid; R.L = e->L; R.pd = e->pd; R.l0 = pl.layers[0]; R.layer_stride = pl.layer_stride(); R.outw = pl.outw; R.outb = pl.outb;
    const BodyPlan& P = e->mode;
    R.fold = P.fold_ln1 || P.fold_ln3; R.fp8 = P.fp8;
#define JOB(ptr, src, n, kind, cols) IMG(ptr, (kind) == RJ_SPLIT_HL ? 2 * (n) : (n)) R.jobs[R.njobs++] = RefreshJob{ptr, src, n, kind, cols};
#define COPY(ptr, src, n) JOB(e->ptr, pl.src, n, RJ_COPY, 0)
    COPY(ff1_w, ff1w, d * ne) COPY(ff1_b, ff1b, d) COPY(ff3_w, ff3w, d * d) COPY(ff3_b, ff3b, d) COPY(label_w, lbw, d * text) COPY(label_b, lbb, d)
    COPY(norm_w, nw, d) COPY(norm_b, nb, d) COPY(conv_w, cvw, pd * pd) COPY(conv_b, cvb, pd) COPY(pln1_w, l1w, pd) COPY(pln1_b, l1b, pd)
    COPY(plin_b, lib, d) COPY(pln2_w, l2w, d) COPY(pln2_b, l2b, d) COPY(pos, pos, N * d) COPY(out_w, outw, pd * d) COPY(out_b, outb, pd)
    JOB(e->out_w_hl, pl.outw, pd * d, RJ_SPLIT_HL, 0)        // hi + lo bf16 halves for the matrix-pipe tail kernel (16 significant bits)
    JOB(e->plin_w_hl, pl.liw, d * pd, RJ_SPLIT_HL, 0)        // the same split of the patch-embedding Linear weight [d, pd] (embed_mfma_kernel)
    JOB(e->plin_wt, pl.liw, d * pd, RJ_TRANSPOSE, (int)pd)   // ... and its transpose [pd, d] for coalesced per-feature reads
#undef COPY
#undef JOB
    static_assert(kRefreshMaxJobs >= 21, "the images outside the blocks");
    // the blocks' images this mode holds (body_block_images: the table the stage hook names them from too)
    const std::vector<BodyImage> images = body_block_images(*e, P);
    for (Layer& Ly : e->layers)
        for (const BodyImage& q : images) {
            if (!q.held) continue;
            char* p = nullptr;
            if (int rc = dev_alloc(e, &p, (size_t)(q.numel() + q.margin) * st_bytes(q.dtype))) return rc;
            q.set(Ly, p);
            e->weight_bytes += q.numel() * (int64_t)st_bytes(q.dtype);
        }
    if (P.fold_tail_held) {   // out_proj folded into the last block's down projection (tld_tail_fold_math.h); rows pd .. pdp - 1 of the image stay zero
        const size_t n = (size_t)(2 * tail_fold_padded_rows((int)pd) * (d + hid));
        IMG(e->mb.out_fold_hl, n) IMG(e->mb.out_fold_b, pd)
        HIP_TRY(hipMemsetAsync(e->mb.out_fold_hl, 0, n * sizeof(bf16), nullptr));
        R.tail_fold_hl = e->mb.out_fold_hl; R.tail_fold_b = e->mb.out_fold_b;
    }
#undef IMG
    {   // per-layer pointer tables for the layer-batched conditioning launches
        const size_t L = (size_t)e->L;
        std::vector<const float*> tab(4 * L);
        for (size_t l = 0; l < L; ++l) { tab[l] = e->layers[l].kv_w; tab[L + l] = e->layers[l].q_w; tab[2 * L + l] = e->layers[l].n2_w; tab[3 * L + l] = e->layers[l].n2_b; }
        const float** tabs = nullptr;
        if (int rc = dev_alloc(e, &tabs, 4 * L)) return rc;
        e->tab_kv_w = tabs; e->tab_q_w = tabs + L; e->tab_n2_w = tabs + 2 * L; e->tab_n2_b = tabs + 3 * L;
        HIP_TRY(hipMemcpy(tabs, tab.data(), 4 * L * sizeof(float*), hipMemcpyHostToDevice));
        Layer* ld = nullptr;      // the blocks' image pointers as a device table (the refresh kernels index it by blockIdx.z)
        if (int rc = dev_alloc(e, &ld, L)) return rc;
        HIP_TRY(hipMemcpy(ld, e->layers.data(), L * sizeof(Layer), hipMemcpyHostToDevice));
        R.layers_dev = ld;
    }
    {   // the loaded values as a temporary flat vector (outside the arena: freed before the activations are allocated), and the one refresh
        struct Flat { float* p = nullptr; ~Flat() { if (p) (void)hipFree(p); } } flat;
        HIP_TRY(hipMalloc(&flat.p, (size_t)pl.count * sizeof(float)));
        for (const ParamTensor& q : pl.tensors)
            HIP_TRY(hipMemcpy(flat.p + q.off, e->host[q.key].data.data(), (size_t)q.numel * sizeof(float), hipMemcpyHostToDevice));
        e->host.clear();
        if (int rc = launch_refresh_weights(R, flat.p, nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(nullptr));
    }

    const size_t B2 = (size_t)e->cfg.max_batch, M = B2 * e->ntok;
    if (int rc = dev_alloc(e, &e->x, M * d)) return rc;
    if (int rc = dev_alloc(e, &e->x_half, M * d)) return rc;      // (up to max_batch - 1 shared samples: a guided call's unconditional subset may be one sample)
    if (int rc = dev_alloc(e, &e->xn, M * d)) return rc;
    if (int rc = dev_alloc(e, &e->row_stats, M + 256)) return rc;
    if (int rc = dev_alloc(e, &e->ln_stats, (M + 256) * kLnSlots)) return rc;
    if (int rc = dev_alloc(e, &e->qk, M * 2 * d)) return rc;
    if (int rc = dev_alloc(e, &e->vt, M * d)) return rc;
    if (int rc = dev_alloc(e, &e->att, M * d)) return rc;
    if (P.pair_held) { if (int rc = dev_alloc(e, &e->mb.pair_park, (size_t)P.pair_slots * kPairSlotDwords)) return rc; }
    if (int rc = dev_alloc(e, &e->hid1, M * hid)) return rc;
    if (P.seam) { if (int rc = dev_alloc(e, &e->mb.seam, M * hid / 4)) return rc; }
    if (int rc = dev_alloc(e, &e->hid2, M * hid)) return rc;
    if (P.fp8) {
        if (int rc = dev_alloc(e, &e->a8, M * hid)) return rc;
        if (int rc = dev_alloc(e, &e->as8, M * hid / 32 + 1024)) return rc;
    }
    {   // what a debug forward poisons first: every activation / statistics / seam buffer above (the split-K slices and the fp8 operand: debug_poison)
        auto& Q = e->poison;
        Q.clear();
        Q.emplace_back(e->x, M * d * sizeof(resid_t)); Q.emplace_back(e->x_half, M * d * sizeof(resid_t)); Q.emplace_back(e->xn, M * d * 2);
        Q.emplace_back(e->row_stats, (M + 256) * sizeof(float2)); Q.emplace_back(e->ln_stats, (M + 256) * kLnSlots * sizeof(float2));
        Q.emplace_back(e->qk, M * 2 * d * 2); Q.emplace_back(e->vt, M * d * 2); Q.emplace_back(e->att, M * d * 2);
        Q.emplace_back(e->hid1, M * hid * 2); Q.emplace_back(e->hid2, M * hid * 2);
        if (P.seam) Q.emplace_back(e->mb.seam, M * hid / 4 * sizeof(uint32_t));
    }
    if (int rc = dev_alloc(e, &e->io_x, B2 * e->img)) return rc;
    if (int rc = dev_alloc(e, &e->io_out, B2 * e->img)) return rc;
    if (int rc = dev_alloc(e, &e->io_sigma, B2)) return rc;
    if (int rc = dev_alloc(e, &e->io_label, B2 * e->text)) return rc;
    if (int rc = dev_alloc(e, &e->xt, B2 * e->img)) return rc;
    if (int rc = dev_alloc(e, &e->x0_prev, B2 * e->img)) return rc;
    if (int rc = ensure_cond_capacity(e, 2 * (int)B2)) return rc;
    if (int rc = dev_alloc(e, &e->rows_dev, 2 * B2)) return rc;
    if (int rc = ensure_req_capacity(e, 64 * (sizeof(SamplerStepRow) + 8 * B2))) return rc;      // a 64-level call at full batch; larger calls grow it
    e->finalized = true;
    return TLD_OK;
}

int64_t tld_engine_param_count(const tld_engine* e) { return e ? e->nparam : 0; }

int tld_engine_refresh_weights(tld_engine* e, const float* flat_device, int64_t numel, void* hip_stream) {
    if (!e || !flat_device) return fail(TLD_ERR_INVALID, "null argument");
    if (!e->finalized) return fail(TLD_ERR_STATE, "tld_engine_refresh_weights: weights not finalized (the first load goes through tld_engine_load_tensor)");
    if (numel != e->nparam)
        return fail(TLD_ERR_SHAPE, "tld_engine_refresh_weights: the flat vector has %lld elements, this configuration %lld", (long long)numel, (long long)e->nparam);
    if (e->session) return fail(TLD_ERR_STATE, "tld_engine_refresh_weights: a sampler session is open on this engine: its conditioning rows were made from the weights it opened with (tld_session_close first)");
    DeviceGuard dg(e->cfg.device_id);
    return launch_refresh_weights(e->refresh, flat_device, static_cast<hipStream_t>(hip_stream));
}

int tld_engine_set_debug(tld_engine* e, int32_t enable) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    DeviceGuard dg(e->cfg.device_id);
    if (enable) {
        if (!e->finalized) return fail(TLD_ERR_STATE, "tld_engine_set_debug: weights not finalized");
        e->debug = true;
        if (int rc = reserve_snapshots(e)) { (void)hipDeviceSynchronize(); e->stages.free_all(); e->debug = false; return rc; }
    } else {
        (void)hipDeviceSynchronize();
        e->stages.free_all();
        e->debug = false; e->dbg_keep = false;
    }
    return TLD_OK;
}

int tld_engine_set_debug_step(tld_engine* e, int32_t step) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    e->dbg_step = step;
    return TLD_OK;
}

int tld_engine_debug_paths(tld_engine* e, uint64_t* mask) {
    if (!e || !mask) return fail(TLD_ERR_INVALID, "null argument");
    *mask = e->paths;
    return TLD_OK;
}

namespace {
// the six stage names of the first hook, and the two hidden-tensor ones
std::string stage_alias(const tld_engine* e, const char* name) {
    const struct { const char* old_name; const char* new_name; } al[] = {{"cond_y", "cond.y"}, {"blk0_sa", "blk0.sa"}, {"blk0_ca", "blk0.ca"},
        {"blk0_mlp", "blk0.mlp"}, {"blk0_hid", "blk0.hid"}, {"blk0_hid_pre", "blk0.hid_pre"}};
    for (const auto& a : al) if (!strcmp(name, a.old_name)) return a.new_name;
    if (!strcmp(name, "tokens_final")) return blk_name(e->L - 1, "mlp");
    return name;
}
}  // namespace

int tld_debug_decode_stage(const void* raw, const void* aux, int32_t dtype, int32_t layout, const int64_t* shape4, int64_t outer_stride, int32_t d,
                           int32_t heads, float* out, int64_t numel) {
    if (!raw || !shape4 || !out) return fail(TLD_ERR_INVALID, "tld_debug_decode_stage: null argument");
    if (numel != stage_numel(shape4)) return fail(TLD_ERR_SHAPE, "tld_debug_decode_stage: the shape has %lld elements, the caller's buffer %lld", (long long)stage_numel(shape4), (long long)numel);
    StageExtra x;
    x.outer_stride = outer_stride; x.d = d; x.heads = heads;
    return decode_stage(raw, aux, dtype, layout, shape4, x, out);
}

int tld_engine_stage_shape(tld_engine* e, const char* name, int64_t* shape4) {
    if (!e || !name || !shape4) return fail(TLD_ERR_INVALID, "null argument");
    return e->stages.read(stage_alias(e, name), nullptr, 0, shape4);
}

int tld_engine_read_stage(tld_engine* e, const char* name, float* host_out, int64_t numel) {
    if (!e || !name || !host_out) return fail(TLD_ERR_INVALID, "null argument");
    DeviceGuard dg(e->cfg.device_id);
    return e->stages.read(stage_alias(e, name), host_out, numel, nullptr);
}

int tld_denoiser_forward(tld_engine* e, const void* x, const void* noise, const void* label, void* out,
                         int32_t batch, int32_t io_dtype, void* hip_stream) {
    if (!e || !x || !noise || !label || !out) return fail(TLD_ERR_INVALID, "null argument");
    if (!e->finalized) return fail(TLD_ERR_STATE, "weights not finalized");
    if (e->session) return fail(TLD_ERR_STATE, "a sampler session is open on this engine: it owns the conditioning tables (tld_session_close first)");
    if (batch <= 0 || batch > e->cfg.max_batch) return fail(TLD_ERR_INVALID, "batch %d outside (0, max_batch=%d]", batch, e->cfg.max_batch);
    if (io_dtype < 0 || io_dtype > 2) return fail(TLD_ERR_INVALID, "bad io_dtype %d", io_dtype);
    DeviceGuard dg(e->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const float* xin = static_cast<const float*>(x);
    float* o = static_cast<float*>(out);
    PathScope paths(e);
    if (int rc = debug_begin(e, 2 * batch, batch, s)) return rc;
    e->dbg_keep = e->debug;
    if (io_dtype != TLD_DTYPE_F32) {
        launch_cast_to_f32(x, io_dtype, e->io_x, (int64_t)batch * e->img, s);
        xin = e->io_x; o = e->io_out;
    }
    // conditioning token rows: [0,batch) noise tokens, [batch, 2*batch) label tokens
    launch_cast_to_f32(noise, io_dtype, e->c_sigma, batch, s);
    launch_cast_to_f32(label, io_dtype, e->c_label, (int64_t)batch * e->text, s);
    {
        ProfScope ps(e, KC_COND, s);
        cond_noise_rows(e, batch, s);
        cond_label_rows(e, batch, batch, s);
    }
    if (int rc = cond_tables(e, 2 * batch, s)) return rc;
    launch_iota(e->rows_dev, 2 * batch, 0, s);
    if (int rc = run_body(e, xin, batch, batch, e->rows_dev, e->rows_dev + batch, o, s)) return rc;
    if (io_dtype != TLD_DTYPE_F32) launch_cast_from_f32(e->io_out, out, io_dtype, (int64_t)batch * e->img, s);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_sample(tld_engine* e, const void* x_T, const void* labels, const float* coeffs, int32_t n_levels,
               float class_guidance, float sharp_f, float bright_f, void* out_latent, int32_t batch,
               void* trace_x0, void* trace_xt, void* hip_stream) {
    if (!e || !x_T || !labels || !coeffs || !out_latent) return fail(TLD_ERR_INVALID, "null argument");
    return run_uniform(e, x_T, nullptr, nullptr, 1.0f, labels, coeffs, n_levels, class_guidance, sharp_f, bright_f, out_latent, batch, trace_x0, trace_xt,
                       EP_UPDATE, hip_stream);
}

int tld_sample_from(tld_engine* e, const void* noise, const void* init_latent, const void* mask, float start_mix, const void* labels,
                    const float* coeffs, int32_t n_levels, float class_guidance, float sharp_f, float bright_f, void* out_latent,
                    int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream) {
    if (!e || !noise || !labels || !coeffs || !out_latent) return fail(TLD_ERR_INVALID, "null argument");
    if (!(start_mix > 0.0f && start_mix <= 1.0f)) return fail(TLD_ERR_INVALID, "start_mix %g outside (0, 1]", (double)start_mix);
    if (!init_latent && (mask || start_mix < 1.0f)) return fail(TLD_ERR_INVALID, "init_latent is required with a mask or with start_mix < 1");
    return run_uniform(e, noise, init_latent, mask, start_mix, labels, coeffs, n_levels, class_guidance, sharp_f, bright_f, out_latent, batch, trace_x0,
                       trace_xt, mask ? EP_UPDATE_FROM_MASK : EP_UPDATE_FROM, hip_stream);
}

int tld_sample_requests(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
                        const tld_sample_request* requests, const float* coeffs, int32_t n_max, float sharp_f, float bright_f, void* out_latent,
                        int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream) {
    return run_requests(SE_REQUESTS, e, noise, init_latent, mask, labels, neg_labels, requests, coeffs, nullptr, nullptr, nullptr, nullptr, n_max, sharp_f,
                        bright_f, out_latent, batch, trace_x0, trace_xt, hip_stream);
}

int tld_sample_requests_guided(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
                               const tld_sample_request* requests, const float* coeffs, const float* guidance, int32_t n_max, float sharp_f,
                               float bright_f, void* out_latent, int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream) {
    return run_requests(SE_GUIDED, e, noise, init_latent, mask, labels, neg_labels, requests, coeffs, guidance, nullptr, nullptr, nullptr, n_max, sharp_f,
                        bright_f, out_latent, batch, trace_x0, trace_xt, hip_stream);
}

int tld_sample_requests_stochastic(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
                                   const tld_sample_request* requests, const float* coeffs, const float* guidance, const float* noise_coeff,
                                   const uint64_t* noise_keys, int32_t n_max, float sharp_f, float bright_f, void* out_latent, int32_t batch,
                                   void* trace_x0, void* trace_xt, void* hip_stream) {
    return run_requests(SE_STOCHASTIC, e, noise, init_latent, mask, labels, neg_labels, requests, coeffs, guidance, noise_coeff, noise_keys, nullptr, n_max,
                        sharp_f, bright_f, out_latent, batch, trace_x0, trace_xt, hip_stream);
}

int tld_sample_requests_shaped(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
                               const tld_sample_request* requests, const float* coeffs, const float* guidance, const float* noise_coeff,
                               const uint64_t* noise_keys, const float* shape, int32_t n_max, float sharp_f, float bright_f, void* out_latent, int32_t batch,
                               void* trace_x0, void* trace_xt, void* hip_stream) {
    return run_requests(SE_SHAPED, e, noise, init_latent, mask, labels, neg_labels, requests, coeffs, guidance, noise_coeff, noise_keys, shape, n_max,
                        sharp_f, bright_f, out_latent, batch, trace_x0, trace_xt, hip_stream);
}

int tld_debug_guidance_shape(const float* cond_device, const float* unc_device, float* mom_device, const float* g, const float* shape, int32_t batch,
                             int32_t img, float* x0_device, float* pq_device, double* sums_device, void* hip_stream) {
    if (!cond_device || !unc_device || !g || !shape || !x0_device || !pq_device || !sums_device) return fail(TLD_ERR_INVALID, "null argument");
    if (batch <= 0 || img <= 0) return fail(TLD_ERR_INVALID, "need positive sizes (batch %d, img %d)", batch, img);
    std::vector<SamplerStepRow> steps((size_t)batch);
    std::vector<GuidanceShape> rows((size_t)batch);
    for (int b = 0; b < batch; ++b) {
        rows[(size_t)b] = GuidanceShape{shape[4 * b], shape[4 * b + 1], shape[4 * b + 2], shape[4 * b + 3]};
        if (const char* bad = guidance_shape_invalid(rows[(size_t)b]))
            return fail(TLD_ERR_INVALID, "entry %d: shape (%g, %g, %g, %g): bad %s", b, (double)shape[4 * b], (double)shape[4 * b + 1], (double)shape[4 * b + 2],
                        (double)shape[4 * b + 3], bad);
        if (!std::isfinite(g[b])) return fail(TLD_ERR_INVALID, "entry %d: guidance %g is not finite", b, (double)g[b]);
        if (!mom_device && rows[(size_t)b].beta != 0.0f)
            return fail(TLD_ERR_INVALID, "entry %d: beta = %g needs the momentum buffer", b, (double)rows[(size_t)b].beta);
        steps[(size_t)b] = SamplerStepRow{};
        steps[(size_t)b].g = g[b];
        steps[(size_t)b].final_step = (b + 1) << 1;           // (entry b's unconditional operand is unc[b]: slot b, as the step kernel packs it)
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t step_bytes = (size_t)batch * sizeof(SamplerStepRow), shape_bytes = (size_t)batch * sizeof(GuidanceShape);
    char* tab = nullptr;
    HIP_TRY(hipMalloc(&tab, step_bytes + shape_bytes));
    int rc = TLD_OK;
    auto run = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(tab, steps.data(), step_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(tab + step_bytes, rows.data(), shape_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(pq_device, 0, (size_t)batch * sizeof(float2), s));
        HIP_TRY(hipMemsetAsync(sums_device, 0, (size_t)batch * GS_SUMS * sizeof(double), s));
        GuidanceStatsParams gp{};
        gp.cond = cond_device; gp.unc_base = unc_device; gp.mom = mom_device; gp.rows = reinterpret_cast<const SamplerStepRow*>(tab);
        gp.shape_rows = reinterpret_cast<const GuidanceShape*>(tab + step_bytes);
        gp.row_stride = 1; gp.active = batch; gp.img = img; gp.pq = reinterpret_cast<float2*>(pq_device); gp.sums = sums_device;
        launch_guidance_stats(gp, s);
        launch_guidance_shape_debug(cond_device, unc_device, mom_device, gp.rows, gp.shape_rows, gp.pq, batch, img, x0_device, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));                      // (the tables are this call's own)
        return TLD_OK;
    };
    rc = run();
    hipFree(tab);
    return rc;
}

int tld_debug_sampler_noise(const uint64_t* keys_device, const uint32_t* steps_device, int32_t batch, int32_t img, float* out_device, void* hip_stream) {
    if (!keys_device || !steps_device || !out_device) return fail(TLD_ERR_INVALID, "null argument");
    if (batch <= 0 || img <= 0) return fail(TLD_ERR_INVALID, "need positive sizes (batch %d, img %d)", batch, img);
    launch_sampler_noise_debug(keys_device, steps_device, batch, img, out_device, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_engine_sample_rows(tld_engine* e, int64_t* cond, int64_t* uncond) {
    if (!e || !cond || !uncond) return fail(TLD_ERR_INVALID, "null argument");
    *cond = e->rows_cond; *uncond = e->rows_uncond;
    return TLD_OK;
}

int tld_debug_gemm_bf16(const void* a, const void* w, float* c, int32_t M, int32_t N, int32_t K, void* hip_stream) {
    if (!a || !w || !c) return fail(TLD_ERR_INVALID, "null argument");
    if (K % 64 || K <= 0 || M <= 0 || N <= 0) return fail(TLD_ERR_INVALID, "need K %% 64 == 0 and positive sizes");
    GemmParams g{};
    g.A = static_cast<const bf16*>(a); g.lda = K; g.W = static_cast<const bf16*>(w); g.ldw = K;
    g.M = M; g.N = N; g.K = K; g.c_f32 = c; g.ldc = N;
    // the launch's own reach check decides: the last A row may start up to 4 GiB - 128 bytes into the operand
    if (launch_gemm(g, EPI_F32, static_cast<hipStream_t>(hip_stream))) return TLD_ERR_INVALID;
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_debug_gemm_splitk(const void* a, const void* w, float* c_slices, int32_t M, int32_t N, int32_t K, int32_t ksplit, void* hip_stream) {
    if (!a || !w || !c_slices) return fail(TLD_ERR_INVALID, "null argument");
    if (ksplit <= 0 || K <= 0 || K % (64 * ksplit) || M <= 0 || N <= 0) return fail(TLD_ERR_INVALID, "need K %% (64 ksplit) == 0 and positive sizes");
    if ((int64_t)M * K * 2 >= (int64_t)1 << 32 || (int64_t)N * K * 2 >= (int64_t)1 << 32) return fail(TLD_ERR_INVALID, "operands must be smaller than 4 GiB");
    GemmParams g{};
    g.A = static_cast<const bf16*>(a); g.lda = K; g.W = static_cast<const bf16*>(w); g.ldw = K;
    g.M = M; g.N = N; g.K = K / ksplit; g.ksplit = ksplit; g.c_f32 = c_slices; g.ldc = N;
    if (launch_gemm(g, EPI_F32, static_cast<hipStream_t>(hip_stream))) return TLD_ERR_INVALID;     // (refused: reason in tld_last_error)
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_debug_gemm_bench(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t ntok, int32_t iters,
                         double* avg_ms) {
    if (!avg_ms || M <= 0 || N <= 0 || K <= 0 || K % 64 || iters <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    if ((int64_t)M * K * 2 >= (int64_t)1 << 32 || (int64_t)N * K * 2 >= (int64_t)1 << 32)
        return fail(TLD_ERR_INVALID, "operands must be smaller than 4 GiB");
    if (epilogue == EPI_QKV && (N % 3 || ntok <= 0 || M % ntok)) return fail(TLD_ERR_INVALID, "QKV epilogue needs N = 3d, M %% ntok == 0");
    bf16 *A = nullptr, *W = nullptr, *out = nullptr, *vt = nullptr;
    float *bias = nullptr, *res = nullptr;   // res doubles as fp32 C and as the residual buffer (sized for fp32)
    HIP_TRY(hipMalloc(&A, (size_t)M * K * 2)); HIP_TRY(hipMalloc(&W, (size_t)N * K * 2));
    HIP_TRY(hipMalloc(&out, (size_t)M * N * 2)); HIP_TRY(hipMalloc(&vt, (size_t)M * N * 2));
    HIP_TRY(hipMalloc(&bias, (size_t)N * 4)); HIP_TRY(hipMalloc(&res, (size_t)M * N * 4));
    const float zs = getenv("TLD_GEMM_ZERO") ? 0.0f : 1.0f;     // DVFS experiment: all-zero operands
    launch_fill_bf16(A, (int64_t)M * K, 1u, 1.0f * zs, nullptr);
    const float wsc = getenv("TLD_GEMM_WSCALE") ? (float)atof(getenv("TLD_GEMM_WSCALE")) : 0.05f;     // 1.0: both operands uniform in [-1, 1) (the GEMM template's benchmark data)
    launch_fill_bf16(W, (int64_t)N * K, 2u, wsc * zs, nullptr);
    HIP_TRY(hipMemset(bias, 0, (size_t)N * 4)); HIP_TRY(hipMemset(res, 0, (size_t)M * N * 4));
    GemmParams g{};
    g.A = A; g.lda = K; g.W = W; g.ldw = K; g.M = M; g.N = N; g.K = K;
    g.c_f32 = res; g.ldc = N; g.out_bf16 = out; g.ldo = epilogue == EPI_QKV ? 2 * (N / 3) : N; g.vt = vt;
    g.ntok = ntok > 0 ? ntok : 1; g.d = N / 3; g.bias = bias; g.resid = reinterpret_cast<resid_t*>(res); g.ldr = N;
    g.dbg_epi = getenv("TLD_EPI_DBG") ? atoi(getenv("TLD_EPI_DBG")) : 0;
    float *dww = nullptr;
    if (epilogue == EPI_UP_DWCONV2) {
        if (M % 256 || N % 256) return fail(TLD_ERR_INVALID, "fused depthwise epilogue needs M, N multiples of 256");
        HIP_TRY(hipMalloc(&dww, (size_t)N * 22 * 4));
        std::vector<float> hw((size_t)N * 22);
        for (size_t i = 0; i < (size_t)N * 10; ++i) hw[i] = 0.05f + 0.01f * (float)(i % 7);
        uint32_t* pk = reinterpret_cast<uint32_t*>(hw.data() + (size_t)N * 10);
        for (size_t i = 0; i < (size_t)N * 12; ++i) pk[i] = 0x3d803d00u + (uint32_t)(i % 5) * 0x00010001u;     // small bf16 pairs
        HIP_TRY(hipMemcpy(dww, hw.data(), hw.size() * 4, hipMemcpyHostToDevice));
        g.dw_b = dww + (size_t)N * 9; g.dw_wpk = reinterpret_cast<const uint32_t*>(dww + (size_t)N * 10);
    }
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
    auto run = [&]() { return launch_gemm(g, epilogue, nullptr); };
    if (const int rc = run()) {      // a refused plan (the reason is in tld_last_error): every later launch would be refused alike, nothing to time
        hipEventDestroy(a); hipEventDestroy(b);
        hipFree(A); hipFree(W); hipFree(out); hipFree(vt); hipFree(bias); hipFree(res); hipFree(dww);
        return rc;
    }
    for (int i = 1; i < 3; ++i) (void)run();
    HIP_TRY(hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) (void)run();
    HIP_TRY(hipEventRecord(b, nullptr));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    *avg_ms = ms / iters;
    hipEventDestroy(a); hipEventDestroy(b);
    hipFree(A); hipFree(W); hipFree(out); hipFree(vt); hipFree(bias); hipFree(res); hipFree(dww);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_engine_set_low_latency(tld_engine* e, int32_t on) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    DeviceGuard dg(e->cfg.device_id);
    if (e->session) return fail(TLD_ERR_STATE, "tld_engine_set_low_latency: a sampler session is open on this engine (tld_session_close first)");
    if (const std::string bad = body_class_refusal(*e, e->cfg.max_batch, on, e->mode.fp8); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    if (const int split = lowlat_split(on)) {
        // (a class-1 buffer is too small for eight slices: allocate anew; the old one is released with the engine)
        if (e->mb.splitk_slices < split) { if (int rc = dev_alloc(e, &e->mb.splitk, (size_t)split * e->cfg.max_batch * e->ntok * e->d)) return rc; }
        e->mb.splitk_slices = split;
    }
    replan(e, e->mode.fp8, on);
    return TLD_OK;
}

int tld_engine_set_gemm_dtype(tld_engine* e, int32_t dtype) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    if (e->finalized) return fail(TLD_ERR_STATE, "the GEMM operand type must be chosen before tld_engine_finalize_weights");
    DeviceGuard dg(e->cfg.device_id);
    if (const std::string bad = body_dtype_refusal(*e, dtype, e->mode.cls); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    body_switches_set_dtype(e->sw, dtype);      // ((1) writes three switches off and (0) does not put them back: kept as it was, see there)
    replan(e, dtype == 1, e->mode.cls);
    return TLD_OK;
}

int tld_debug_quant_mx8_host(const float* w, int32_t rows, int32_t K, void* out_e4m3, void* out_scale) {
    if (!w || !out_e4m3 || !out_scale || rows <= 0 || K <= 0 || K % 128) return fail(TLD_ERR_INVALID, "bad argument (K %% 128 == 0)");
    quant_mx8_host(w, rows, K, static_cast<uint8_t*>(out_e4m3), static_cast<uint8_t*>(out_scale));
    return TLD_OK;
}

int tld_debug_quant_mx8(const void* in_bf16, void* out_e4m3, void* out_scale, int32_t M, int32_t K, void* hip_stream) {
    if (!in_bf16 || !out_e4m3 || !out_scale || M <= 0 || K <= 0 || K % 128) return fail(TLD_ERR_INVALID, "bad argument (K %% 128 == 0)");
    PtrDeviceGuard guard(in_bf16);
    launch_quant_mx8(static_cast<const bf16*>(in_bf16), static_cast<uint8_t*>(out_e4m3), static_cast<uint8_t*>(out_scale), M, K,
                     static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_debug_quant_mx8_f32(const float* in_device, void* out_e4m3, void* out_scale, int32_t rows, int32_t K, void* hip_stream) {
    if (!in_device || !out_e4m3 || !out_scale || rows <= 0 || K <= 0 || K % 128) return fail(TLD_ERR_INVALID, "bad argument (K %% 128 == 0)");
    PtrDeviceGuard guard(in_device);
    launch_quant_mx8_f32(in_device, static_cast<uint8_t*>(out_e4m3), static_cast<uint8_t*>(out_scale), rows, K, static_cast<hipStream_t>(hip_stream));
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_debug_gemm_mx8(const void* a_e4m3, const void* a_scale, const void* w_e4m3, const void* w_scale, float* c, int32_t M,
                       int32_t N, int32_t K, void* hip_stream) {
    if (!a_e4m3 || !a_scale || !w_e4m3 || !w_scale || !c) return fail(TLD_ERR_INVALID, "null argument");
    if (K % 128 || K <= 0 || M <= 0 || N <= 0 || M % 4 || N % 4) return fail(TLD_ERR_INVALID, "need K %% 128 == 0, M %% 4 == 0, N %% 4 == 0");
    PtrDeviceGuard guard(a_e4m3);
    GemmParams g{};
    g.f8 = 1;
    g.A = static_cast<const bf16*>(a_e4m3); g.lda = K; g.W = static_cast<const bf16*>(w_e4m3); g.ldw = K;
    g.a_scale = static_cast<const uint8_t*>(a_scale); g.w_scale = static_cast<const uint8_t*>(w_scale);
    g.M = M; g.N = N; g.K = K; g.c_f32 = c; g.ldc = N;
    if (launch_gemm(g, EPI_F32, static_cast<hipStream_t>(hip_stream))) return TLD_ERR_INVALID;     // (refused: reason in tld_last_error)
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

// One launch_gemm call on the caller's buffers, any non-conv epilogue: what the kernels assume silently is checked here, nothing else is added.
int tld_debug_gemm_epilogue(const tld_gemm_epilogue_args* a, void* hip_stream) {
    if (!a) return fail(TLD_ERR_INVALID, "tld_debug_gemm_epilogue: null argument");
    auto bad = [](const char* why) { return fail(TLD_ERR_INVALID, "tld_debug_gemm_epilogue: %s", why); };
    auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    const int epi = a->epilogue;
    const bool f8 = a->f8 != 0;
    if (epi != EPI_F32 && epi != EPI_QKV && epi != EPI_BIAS_BF16 && epi != EPI_BIAS_RESID && epi != EPI_QKV_LN)
        return bad("epilogue must be 0 (fp32), 1 (QKV), 2 (bias -> bf16), 3 (bias + residual add) or 5 (QKV with LayerNorm-1); the fused depthwise and attention "
                   "epilogues and convolution mode have engine-internal layouts and tests of their own");
    if (f8 && epi == EPI_QKV_LN) return bad("the LayerNorm-1 fold has no fp8 form");
    if (!a->A || !a->W || a->M <= 0 || a->N <= 0 || a->K <= 0) return bad("A, W and positive M, N, K are needed");
    // operands: 128-byte K-steps, rows fetched in 16-byte pieces
    const int esz = f8 ? 1 : 2;
    if (a->K % (f8 ? 128 : 64)) return bad("K must be a multiple of 64 (fp8: 128)");
    if (a->lda < a->K || a->ldw < a->K || (a->lda * esz) % 16 || (a->ldw * esz) % 16 || !al16(a->A) || !al16(a->W))
        return bad("lda, ldw >= K, operand rows and pointers 16-byte aligned");
    if (f8 && (!a->a_scale || !a->w_scale || a->M % 4 || a->N % 4 || !al16(a->a_scale) || !al16(a->w_scale)))
        return bad("fp8 operands need both scale arrays (16-byte aligned), M % 4 == 0 and N % 4 == 0");
    if (a->w_batch_rows) {
        if (f8 || (epi != EPI_F32 && epi != EPI_BIAS_BF16) || a->w_batch_rows < 0 || a->w_batch_rows % 256 || a->w_batch_stride_bytes % 16)
            return bad("w_batch_rows: bf16 operands, epilogues 0 and 2 only, a multiple of 256 rows, a 16-byte aligned stride");
    }
    if (epi == EPI_F32) {
        if (!a->c_f32 || a->ldc < a->N) return bad("epilogue 0 needs c_f32 and ldc >= N");
    } else if (epi == EPI_BIAS_RESID) {
        // float4 of bias and four residual values (8 bytes) per lane, the column predicate on the first of the four
        if (!a->bias || !a->resid || !al16(a->bias) || (reinterpret_cast<uintptr_t>(a->resid) & 7)) return bad("epilogue 3 needs bias (16-byte aligned) and resid (8-byte aligned)");
        if (a->N % 4 || a->ldr % 4 || a->ldr < a->N) return bad("epilogue 3 needs N % 4 == 0, ldr % 4 == 0 and ldr >= N");
        // partial sums are taken by the 96-column wave tiles only (192- / 384-wide tiles, the 4-wave form); any other launch would leave stats_out unwritten
        if (a->stats_out && (f8 || gemm_resid_stat_slots(a->N) == 0)) return bad("stats_out: bf16 operands and N % 192 == 0, N <= 768 only (one slot per 96 columns, at most 8)");
        if (a->stats_out && (reinterpret_cast<uintptr_t>(a->stats_out) & 7)) return bad("stats_out must be 8-byte aligned");
    } else {
        // bf16-storing epilogues: 16-byte groups of 8 columns, the column predicate on the first; bias / c1 / b1 as float4
        if (!a->out_bf16 || !al16(a->out_bf16) || a->N % 8 || a->ldo % 8) return bad("epilogues 1, 2, 5 need out_bf16 (16-byte aligned), N % 8 == 0 and ldo % 8 == 0");
        if (epi == EPI_BIAS_BF16) {
            if (!a->bias || !al16(a->bias) || a->ldo < a->N) return bad("epilogue 2 needs bias (16-byte aligned) and ldo >= N");
            if (a->row_stats) {
                if (!a->ln_c1 || !al16(a->ln_c1) || !al16(a->row_stats)) return bad("row_stats needs ln_c1, both 16-byte aligned");
                if (f8) return bad("row_stats: the LayerNorm-3 fold has no fp8 form");
                if (a->M % 2) return bad("row_stats: M must be even (the statistics are fetched two rows at a time)");
                if (a->N % 384 == 0 && a->N < 1536) return bad("row_stats: the 384-wide tile, which N % 384 == 0 below 1536 may get, has no LayerNorm-3 fold");
            }
        } else {
            // one tile is q | k or v, never both: 2 d is a multiple of the tile width (256-wide tiles need N % 256 == 0, and then 2 d % 256 == 0 follows from
            // d % 64 == 0); a V^T store is 8 tokens of one sample
            if (!a->vt || !al16(a->vt) || a->d <= 0 || a->d % 64 || a->N != 3 * a->d) return bad("QKV epilogues need vt (16-byte aligned), d % 64 == 0 and N = 3 d");
            if (a->ntok <= 0 || a->ntok % 8 || a->M % a->ntok) return bad("QKV epilogues need ntok % 8 == 0 and M % ntok == 0");
            if (a->ldo < 2 * a->d) return bad("QKV epilogues need ldo >= 2 d");
            if (epi == EPI_QKV_LN) {
                if (!a->ln_stats || !a->ln_c1 || !a->ln_b1 || !al16(a->ln_stats) || !al16(a->ln_c1) || !al16(a->ln_b1)) return bad("epilogue 5 needs ln_stats, ln_c1 and ln_b1, 16-byte aligned");
                if (a->ln_slots < 2 || a->ln_slots > kLnSlots || a->ln_slots % 2) return bad("ln_slots must be even, 2 .. 8");
            }
        }
    }
    GemmParams g{};
    g.A = static_cast<const bf16*>(a->A); g.lda = a->lda; g.W = static_cast<const bf16*>(a->W); g.ldw = a->ldw;
    g.M = a->M; g.N = a->N; g.K = a->K;
    g.f8 = f8 ? 1 : 0; g.a_scale = static_cast<const uint8_t*>(a->a_scale); g.w_scale = static_cast<const uint8_t*>(a->w_scale);
    g.bias = a->bias;
    g.out_bf16 = static_cast<bf16*>(a->out_bf16); g.ldo = a->ldo;
    g.vt = static_cast<bf16*>(a->vt); g.ntok = a->ntok; g.d = a->d;
    g.resid = static_cast<resid_t*>(a->resid); g.ldr = a->ldr; g.stats_out = static_cast<float2*>(a->stats_out);
    g.ln_stats = static_cast<const float2*>(a->ln_stats); g.ln_slots = a->ln_slots; g.ln_c1 = a->ln_c1; g.ln_b1 = a->ln_b1;
    g.row_stats = static_cast<const float2*>(a->row_stats);
    g.c_f32 = a->c_f32; g.ldc = a->ldc;
    g.w_batch_rows = a->w_batch_rows; g.w_batch_stride_bytes = a->w_batch_stride_bytes;
    if (const std::string reach = gemm_hook_refusal(g); !reach.empty()) return fail(TLD_ERR_INVALID, "%s", reach.c_str());      // (before the device is touched)
    PtrDeviceGuard guard(a->A);
    if (launch_gemm(g, epi, static_cast<hipStream_t>(hip_stream))) return TLD_ERR_INVALID;     // (refused: reason in tld_last_error)
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_engine_set_profile(tld_engine* e, uint32_t class_mask) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    for (int k = 0; k < KC_COUNT; ++k) e->prof_used[k] = 0;       // recorded pairs are forgotten, the pool is kept
    e->prof_mask = class_mask;
    return TLD_OK;
}

int tld_engine_profile_reserve(tld_engine* e, int32_t kclass, int64_t launches) {
    if (!e) return fail(TLD_ERR_INVALID, "null engine");
    if (kclass < 0 || kclass >= KC_COUNT || launches < 0) return fail(TLD_ERR_INVALID, "bad kernel class %d / count", kclass);
    DeviceGuard dg(e->cfg.device_id);
    auto& pool = e->prof_ev[kclass];
    while ((int64_t)pool.size() < launches) {
        hipEvent_t a = nullptr, b = nullptr;
        HIP_TRY(hipEventCreate(&a)); HIP_TRY(hipEventCreate(&b));
        pool.emplace_back(a, b);
    }
    return TLD_OK;
}

int tld_engine_get_profile(tld_engine* e, int32_t kclass, double* total_ms, int64_t* launches) {
    if (!e || !total_ms || !launches) return fail(TLD_ERR_INVALID, "null argument");
    if (kclass < 0 || kclass >= KC_COUNT) return fail(TLD_ERR_INVALID, "bad kernel class %d", kclass);
    DeviceGuard dg(e->cfg.device_id);
    HIP_TRY(hipDeviceSynchronize());
    double tot = 0.0;
    for (size_t i = 0; i < e->prof_used[kclass]; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, e->prof_ev[kclass][i].first, e->prof_ev[kclass][i].second));
        tot += ms;
    }
    *total_ms = tot;
    *launches = (int64_t)e->prof_used[kclass];
    return TLD_OK;
}

int64_t tld_engine_weight_bytes(const tld_engine* e) { return e ? e->weight_bytes : 0; }

int tld_debug_dwconv_gelu(const void* in, const float* weight, const float* bias, void* out, int32_t batch, int32_t grid, int32_t channels,
                          void* hip_stream) {
    if (!in || !weight || !bias || !out || batch <= 0 || grid <= 0 || channels <= 0 || channels % 64) return fail(TLD_ERR_INVALID, "bad argument");
    if (grid % 4) return fail(TLD_ERR_INVALID, "token count %lld unsupported: image_size / patch_size must be a multiple of 4", (long long)grid * grid);     // (body_config_check's rule and words)
    if (const std::string bad = dwconv_hook_refusal(batch, grid, channels); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    PtrDeviceGuard guard(in);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t nc = (size_t)channels;
    std::vector<float> tab(nc * 20);                       // [9][C] taps | [C] bias | the same halved
    for (size_t c = 0; c < nc; ++c) {
        for (int k = 0; k < 9; ++k) { tab[k * nc + c] = weight[c * 9 + k]; tab[nc * 10 + k * nc + c] = 0.5f * weight[c * 9 + k]; }
        tab[9 * nc + c] = bias[c]; tab[nc * 19 + c] = 0.5f * bias[c];
    }
    float* d = nullptr;
    HIP_TRY(hipMalloc(&d, tab.size() * sizeof(float)));
    HIP_TRY(hipMemcpy(d, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    launch_dwconv_gelu(static_cast<const bf16*>(in), static_cast<bf16*>(out), d, d + 9 * nc, d + 10 * nc, d + 19 * nc, batch, grid, channels, s,
                       nullptr, nullptr);
    HIP_TRY(hipStreamSynchronize(s));
    (void)hipFree(d);
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_debug_attention_fwd(const void* qk, const void* vt, void* att, int32_t batch, int32_t ntok, int32_t heads, int32_t iters,
                            float* ms_per_launch, void* hip_stream) {
    if (!qk || !vt || !att || batch <= 0 || heads <= 0 || iters <= 0) return fail(TLD_ERR_INVALID, "bad argument");
    if (ntok <= 0 || ntok % 8 != 0)
        return fail(TLD_ERR_INVALID, "attention supports token counts that are multiples of 8 (got %d)", ntok);
    if (const std::string bad = attention_fwd_hook_refusal(batch, ntok, heads); !bad.empty()) return fail(TLD_ERR_INVALID, "%s", bad.c_str());
    PtrDeviceGuard guard(qk);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    HIP_TRY(hipEventRecord(e0, s));
    for (int i = 0; i < iters; ++i)
        launch_attention(static_cast<const bf16*>(qk), static_cast<const bf16*>(vt), static_cast<bf16*>(att), batch, ntok, heads, s);
    HIP_TRY(hipEventRecord(e1, s));
    HIP_TRY(hipEventSynchronize(e1));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    if (ms_per_launch) *ms_per_launch = ms / (float)iters;
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

}  // extern "C"

// ================================================================================================
// Sampler sessions: the host state is tld_session_plan.h; here the buffers, the new conditioning rows of an admit and the step
struct tld_session {
    tld_engine* e = nullptr;
    hipStream_t stream = nullptr;
    float sharp = 0.0f, bright = 0.0f;
    SessionPlan plan;
    SessionStep st;
    SessionAdmit ad;
    float *xt = nullptr, *x0_prev = nullptr, *out = nullptr;      // [slots, img] each, slot-major
    // a ring of pinned staging buffers, each behind its own event: the host waits only when it laps the ring
    static constexpr int kRing = 4;
    void* stage[kRing] = {};
    hipEvent_t ev[kRing] = {};
    bool used[kRing] = {};
    int head = 0;
    size_t stage_bytes = 0;
};

namespace {

// the next staging buffer of the ring; session_staged after the last copy out of it
int session_stage(tld_session* S, int* k_out) {
    const int k = S->head;
    S->head = (k + 1) % tld_session::kRing;
    if (S->used[k]) HIP_TRY(hipEventSynchronize(S->ev[k]));
    *k_out = k;
    return TLD_OK;
}
int session_staged(tld_session* S, int k) {
    HIP_TRY(hipEventRecord(S->ev[k], S->stream));
    S->used[k] = true;
    return TLD_OK;
}

// admit and step: the session's own stream, not capturing
int session_stream_check(tld_session* S, void* hip_stream) {
    if (static_cast<hipStream_t>(hip_stream) != S->stream) return fail(TLD_ERR_INVALID, "a session runs on the stream it was opened with: this call names another");
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(S->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(TLD_ERR_STATE, "a sampler session cannot be captured into a graph: its membership changes between steps");
    return TLD_OK;
}

// Conditioning of rows r0 .. r0 + n - 1 in place: the launchers of run_sampler pointed at a row range (a row's values depend neither on where it sits nor on
// how many rows the launch carries).  kind: SR_SIGMA from c_sigma, SR_LABEL / SR_ZERO from c_label; then LayerNorm, per-layer K|V and the folded query vectors
void session_cond_rows(tld_engine* e, int kind, int r0, int n, hipStream_t s) {
    const size_t d = e->d, cap = (size_t)e->cond_cap, H = e->H, ne = e->ne, text = e->text;
    float* pre = e->c_pre + (size_t)r0 * d;
    if (kind == SR_SIGMA) {
        launch_sinusoid(e->c_sigma + r0, e->angular, e->c_sin + (size_t)r0 * ne, n, e->ne / 2, s);
        launch_linear_f32(e->c_sin + (size_t)r0 * ne, e->ne, e->ff1_w, e->ff1_b, e->c_h1 + (size_t)r0 * d, e->d, n, e->ne, e->d, 1, s);
        launch_linear_f32(e->c_h1 + (size_t)r0 * d, e->d, e->ff3_w, e->ff3_b, pre, e->d, n, e->d, e->d, 0, s);
    } else {
        launch_linear_f32(e->c_label + (size_t)r0 * text, e->text, e->label_w, e->label_b, pre, e->d, n, e->text, e->d, 0, s);
    }
    launch_layernorm_f32(pre, e->norm_w, e->norm_b, e->c_y + (size_t)r0 * d, n, e->d, s);
    launch_linear_f32_layers(e->c_y + (size_t)r0 * d, e->d, e->tab_kv_w, e->c_kv + (size_t)r0 * 2 * d, cap * 2 * d, 2 * e->d, n, e->d, 2 * e->d, e->L, s);
    launch_wq_layers(e->c_kv + (size_t)r0 * 2 * d, cap * 2 * d, 2 * e->d, e->tab_q_w, e->tab_n2_w, e->tab_n2_b, e->c_wq + (size_t)r0 * H * d, cap * H * d,
                     e->c_bwq + (size_t)r0 * H, cap * H, n, e->H, e->d, e->L, s);
}

void session_free(tld_session* S) {
    for (int k = 0; k < tld_session::kRing; ++k) {
        if (S->ev[k]) (void)hipEventDestroy(S->ev[k]);
        if (S->stage[k]) (void)hipHostFree(S->stage[k]);
    }
    delete S;
}

}  // namespace

extern "C" {

int tld_session_open(tld_engine* e, int32_t slots, int32_t cond_rows, float sharp_f, float bright_f, void* hip_stream, tld_session** out) {
    if (!e || !out) return fail(TLD_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!e->finalized) return fail(TLD_ERR_STATE, "weights not finalized");
    if (e->session) return fail(TLD_ERR_STATE, "a sampler session is already open on this engine: one session per engine");
    if (SampleRefusal r = session_open_check(slots, cond_rows, e->cfg.max_batch)) return fail(r.code, "%s", r.msg.c_str());
    DeviceGuard dg(e->cfg.device_id);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
        return fail(TLD_ERR_STATE, "a sampler session cannot be captured into a graph: its membership changes between steps");
    tld_session* S = new tld_session();
    S->e = e; S->stream = s; S->sharp = sharp_f; S->bright = bright_f;
    S->plan.open(slots, cond_rows, e->mode.guidance_skip);
    auto setup = [&]() -> int {
        if (int rc = ensure_cond_capacity(e, cond_rows)) return rc;
        if (int rc = ensure_req_capacity(e, S->plan.max_up_bytes())) return rc;
        if (slots > e->sess_slots) {      // (grow-only, like every buffer of the arena)
            if (int rc = dev_alloc(e, &e->sess_buf, (size_t)3 * slots * e->img)) return rc;
            e->sess_slots = slots;
        }
        S->xt = e->sess_buf; S->x0_prev = S->xt + (size_t)slots * e->img; S->out = S->x0_prev + (size_t)slots * e->img;
        S->stage_bytes = (std::max(S->plan.max_up_bytes(), (size_t)cond_rows * sizeof(float)) + 4095) & ~(size_t)4095;
        for (int k = 0; k < tld_session::kRing; ++k) {
            HIP_TRY(hipHostMalloc(&S->stage[k], S->stage_bytes, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&S->ev[k], hipEventDisableTiming));
        }
        // row 0: the zero label (diffusion.py:61)
        HIP_TRY(hipMemsetAsync(e->c_label, 0, (size_t)e->text * sizeof(float), s));
        {
            ProfScope ps(e, KC_COND, s);
            session_cond_rows(e, SR_ZERO, 0, 1, s);
        }
        HIP_TRY(hipGetLastError());
        return TLD_OK;
    };
    if (int rc = setup()) { session_free(S); return rc; }
    e->session = S;
    *out = S;
    return TLD_OK;
}

int tld_session_admit(tld_session* S, const tld_session_request* r, void* hip_stream, int32_t* slot_out) {
    // the record first: its checks need no session and no device
    if (SampleRefusal bad = session_request_check(r)) return fail(bad.code, "%s", bad.msg.c_str());
    if (!S || !slot_out || !r->noise || !r->label) return fail(TLD_ERR_INVALID, "null argument");
    *slot_out = -1;
    tld_engine* e = S->e;
    DeviceGuard dg(e->cfg.device_id);
    if (int rc = session_stream_check(S, hip_stream)) return rc;
    if (SampleRefusal bad = session_admit(S->plan, *r, S->ad)) return fail(bad.code, "%s", bad.msg.c_str());
    const SessionAdmit& ad = S->ad;
    if (ad.slot < 0) return TLD_OK;      // no room now
    hipStream_t s = S->stream;
    const size_t img = (size_t)e->img, text = (size_t)e->text;
    HIP_TRY(hipMemcpyAsync(S->xt + (size_t)ad.slot * img, r->noise, img * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(S->x0_prev + (size_t)ad.slot * img, 0, img * sizeof(float), s));
    HIP_TRY(hipMemcpyAsync(e->c_label + (size_t)ad.label_row * text, r->label, text * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (ad.neg_row >= 0) HIP_TRY(hipMemcpyAsync(e->c_label + (size_t)ad.neg_row * text, r->neg_label, text * sizeof(float), hipMemcpyDeviceToDevice, s));
    const size_t ns = ad.new_sigma.size();
    if (ns) {      // the new sigmas through a staging buffer of the ring, one copy and one set of launches per contiguous run of rows
        int k = 0;
        if (int rc = session_stage(S, &k)) return rc;
        float* sig = static_cast<float*>(S->stage[k]);
        for (size_t j = 0; j < ns; ++j) sig[j] = ad.new_sigma[j].second;
        for (size_t j = 0; j < ns; ) {
            size_t j1 = j + 1;
            while (j1 < ns && ad.new_sigma[j1].first == ad.new_sigma[j1 - 1].first + 1) ++j1;
            HIP_TRY(hipMemcpyAsync(e->c_sigma + ad.new_sigma[j].first, sig + j, (j1 - j) * sizeof(float), hipMemcpyHostToDevice, s));
            j = j1;
        }
        if (int rc = session_staged(S, k)) return rc;
    }
    {
        ProfScope ps(e, KC_COND, s);
        for (size_t j = 0; j < ns; ) {
            size_t j1 = j + 1;
            while (j1 < ns && ad.new_sigma[j1].first == ad.new_sigma[j1 - 1].first + 1) ++j1;
            session_cond_rows(e, SR_SIGMA, ad.new_sigma[j].first, (int)(j1 - j), s);
            j = j1;
        }
        if (ad.neg_row == ad.label_row + 1) session_cond_rows(e, SR_LABEL, ad.label_row, 2, s);
        else {
            session_cond_rows(e, SR_LABEL, ad.label_row, 1, s);
            if (ad.neg_row >= 0) session_cond_rows(e, SR_LABEL, ad.neg_row, 1, s);
        }
    }
    HIP_TRY(hipGetLastError());
    *slot_out = ad.slot;
    return TLD_OK;
}

int tld_session_step(tld_session* S, void* hip_stream, int32_t* finished_slots, int32_t cap, int32_t* n_finished) {
    if (!S || !finished_slots || !n_finished) return fail(TLD_ERR_INVALID, "null argument");
    *n_finished = 0;
    if (cap < S->plan.slots) return fail(TLD_ERR_INVALID, "finished_slots has room for %d slots: a step of this session may finish %d", cap, S->plan.slots);
    tld_engine* e = S->e;
    DeviceGuard dg(e->cfg.device_id);
    if (int rc = session_stream_check(S, hip_stream)) return rc;
    if (!S->plan.live) return TLD_OK;      // nothing to run: nothing is enqueued
    hipStream_t s = S->stream;
    int k = 0;
    if (int rc = session_stage(S, &k)) return rc;
    SessionStep& st = S->st;
    session_step(S->plan, st, S->stage[k]);
    for (size_t j = 0; j < st.finished.size(); ++j) finished_slots[j] = st.finished[j];
    *n_finished = (int32_t)st.finished.size();
    HIP_TRY(hipMemcpyAsync(e->req_dev, S->stage[k], st.up_bytes, hipMemcpyHostToDevice, s));      // the one upload of the step
    if (int rc = session_staged(S, k)) return rc;
    const char* dev = static_cast<const char*>(e->req_dev);
    const int Bi = st.Bi, mb = st.mb;
    const int *rs = reinterpret_cast<const int*>(dev + st.ints_off), *nr = rs + Bi, *lr = nr + mb, *sr = lr + mb, *es = sr + mb;
    PathScope paths(e);                      // (debug: the launch paths are recorded and no stage is kept, as for the requests entries)
    if (e->debug) e->paths = 0;
    if (int rc = run_body(e, S->xt, Bi, mb, nr, lr, e->io_out, s, true, sr, es)) return rc;
    SamplerStepParams up{};
    up.x0_2b = e->io_out; up.x_t = S->xt; up.x0_prev = S->x0_prev; up.out_latent = S->out;
    up.rows = reinterpret_cast<const SamplerStepRow*>(dev); up.row_stride = 1; up.sharp = S->sharp; up.bright = S->bright;
    up.active = Bi; up.img = e->img; up.chan_stride = e->cfg.image_size * e->cfg.image_size;
    if (st.noise) up.noise_rows = reinterpret_cast<const SamplerNoiseRow*>(dev + st.noise_off);
    up.req_slot = rs;
    {
        ProfScope ps(e, KC_UPDATE, s);
        launch_sampler_step(up, EP_UPDATE_SESSION, s, true);
    }
    HIP_TRY(hipGetLastError());
    return TLD_OK;
}

int tld_session_latent(tld_session* S, int32_t slot, const float** device_ptr) {
    if (!S || !device_ptr) return fail(TLD_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= S->plan.slots) return fail(TLD_ERR_INVALID, "slot %d outside [0, %d)", slot, S->plan.slots);
    *device_ptr = S->out + (size_t)slot * S->e->img;
    return TLD_OK;
}

int tld_session_copy_latent(tld_session* S, int32_t slot, void* dst_device, void* hip_stream) {
    if (!S || !dst_device) return fail(TLD_ERR_INVALID, "null argument");
    if (slot < 0 || slot >= S->plan.slots) return fail(TLD_ERR_INVALID, "slot %d outside [0, %d)", slot, S->plan.slots);
    DeviceGuard dg(S->e->cfg.device_id);
    if (int rc = session_stream_check(S, hip_stream)) return rc;
    HIP_TRY(hipMemcpyAsync(dst_device, S->out + (size_t)slot * S->e->img, (size_t)S->e->img * sizeof(float), hipMemcpyDeviceToDevice, S->stream));
    return TLD_OK;
}

int tld_session_stats(const tld_session* S, int64_t* out) {
    if (!S || !out) return fail(TLD_ERR_INVALID, "null argument");
    out[0] = S->plan.live; out[1] = S->plan.steps; out[2] = S->plan.rows_cond; out[3] = S->plan.rows_uncond; out[4] = S->plan.rows_used;
    return TLD_OK;
}

int tld_session_close(tld_session* S) {
    if (!S) return TLD_OK;
    tld_engine* e = S->e;
    DeviceGuard dg(e->cfg.device_id);
    for (int k = 0; k < tld_session::kRing; ++k)
        if (S->used[k]) (void)hipEventSynchronize(S->ev[k]);      // (the copies out of the pinned buffers have run before they are freed)
    e->session = nullptr;
    session_free(S);
    return TLD_OK;
}

int tld_engine_destroy(tld_engine* e) {
    if (!e) return TLD_OK;
    if (e->session) (void)tld_session_close(e->session);
    DeviceGuard dg(e->cfg.device_id);
    (void)hipDeviceSynchronize();
    for (int k = 0; k < KC_COUNT; ++k)
        for (auto& ev : e->prof_ev[k]) { hipEventDestroy(ev.first); hipEventDestroy(ev.second); }
    e->stages.free_all();
    for (void* p : e->allocs) (void)hipFree(p);
    if (e->stage_host) (void)hipHostFree(e->stage_host);
    if (e->stage_ev) (void)hipEventDestroy(e->stage_ev);
    delete e;
    return TLD_OK;
}

}  // extern "C"

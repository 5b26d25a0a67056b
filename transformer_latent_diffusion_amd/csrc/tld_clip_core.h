// tld_clip_core.h -- the transformer both CLIP towers are (tld_clip.hip: text, tld_clip_vision.hip: image), host side: what an engine owns, how
// its weights arrive, its stage hook and the launch sequence of its blocks.  A tower adds its front end (what fills x), its attention launch, which
// row of a sample is pooled, and its C entry points.  Include after tld_common.h, tld_host.h and tld_clip_kernels.h; internal linkage, as there.
#pragma once

#include <map>
#include <string>
#include <vector>

#include "tld_clip_keys.h"
#include "tld_reach.h"             // clip_reach_check: the sizes the GEMM DMA's 32-bit offsets and the attention grid end at

namespace tld {
namespace {

struct Block {
    float *ln1_g = nullptr, *ln1_b = nullptr, *ln2_g = nullptr, *ln2_b = nullptr;
    bf16 *in_w = nullptr, *out_w = nullptr, *fc_w = nullptr, *proj_w = nullptr;
    float *in_b = nullptr, *out_b = nullptr, *fc_b = nullptr, *proj_b = nullptr;
};

struct ClipCore : DeviceArena {
    int W = 0, L = 0, H = 0, E = 0, max_batch = 0, device_id = 0;
    bool finalized = false;
    std::map<std::string, HostTensor> host;
    std::vector<Block> blocks;
    float* proj_t = nullptr;                  // the output projection transposed, [E][W]
    // workspace (max_batch * rows-per-sample rows)
    float *x = nullptr, *tmp = nullptr, *pooled = nullptr;
    bf16 *h = nullptr, *qkv = nullptr, *att = nullptr, *f = nullptr;
    // stage capture (set_debug): snapshot memory for max_batch samples, allocated by set_debug(1), freed by set_debug(0) / destroy
    bool debug = false;
    StageStore stages;                        // the stage hook (tld_host.h); the operands are named in it from finalize_weights on
};

// ---- create ------------------------------------------------------------------------------------------------------------------

// the limits both towers have: the transformer's before a tower's own geometry, the device after it.  `tower`: "text" / "image"
int check_transformer(int width, int heads, int layers) {
    if (width < 64 || width > 1024 || width % 64) return fail(TLD_ERR_INVALID, "width=%d: a multiple of 64 in 64..1024", width);
    if (heads * 64 != width) return fail(TLD_ERR_INVALID, "heads=%d: head_dim must be 64 (width / heads)", heads);
    if (layers < 1 || layers > 64) return fail(TLD_ERR_INVALID, "layers=%d: 1..64", layers);
    return TLD_OK;
}
int check_device(int device_id, const char* tower) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TLD_ERR_HIP, "no HIP device available (the %s tower has no CPU path)", tower);
    if (device_id < 0 || device_id >= ndev) return fail(TLD_ERR_INVALID, "device_id=%d out of range (%d devices)", device_id, ndev);
    return TLD_OK;
}
// the workspace of max_batch samples of `rows` rows; a tower's own bf16 buffer (`extra`: the image tower's patches) sits between the fp32 and the bf16 ones
int alloc_workspace(ClipCore* c, int rows, bf16** extra = nullptr, size_t extra_count = 0) {
    const size_t B = (size_t)c->max_batch, T = B * rows, W = c->W;
    if (int rc = dev_alloc(c, &c->x, T * W)) return rc;
    if (int rc = dev_alloc(c, &c->tmp, T * W)) return rc;
    if (int rc = dev_alloc(c, &c->pooled, B * W)) return rc;
    if (extra) { if (int rc = dev_alloc(c, extra, extra_count)) return rc; }
    if (int rc = dev_alloc(c, &c->h, T * W)) return rc;
    if (int rc = dev_alloc(c, &c->qkv, T * 3 * W)) return rc;
    if (int rc = dev_alloc(c, &c->att, T * W)) return rc;
    return dev_alloc(c, &c->f, T * 4 * W);
}

// ---- weights -----------------------------------------------------------------------------------------------------------------

int load_tensor(ClipCore* c, ClipTower tower, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype) {
    if (!c || !key || (!host_ptr && ndim > 0) || (!shape && ndim > 0) || ndim < 0 || ndim > 8) return fail(TLD_ERR_INVALID, "bad argument");
    if (c->finalized) return fail(TLD_ERR_STATE, "weights already finalized");
    std::string k(key);
    const ClipKey whose = route_clip_key(tower, k);
    if (whose == CLIP_KEY_OTHER || whose == CLIP_KEY_METADATA) return TLD_OK;       // the other tower and the archive's metadata are not used by this one
    if (whose == CLIP_KEY_UNKNOWN) return fail(TLD_ERR_KEY, "unknown state_dict key '%s'", key);
    if (dtype != TLD_DTYPE_F32) return fail(TLD_ERR_INVALID, "'%s': host tensors must be fp32", key);
    HostTensor t;
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) { if (shape[i] < 0) return fail(TLD_ERR_SHAPE, "'%s': negative dimension", key); t.shape.push_back(shape[i]); n *= shape[i]; }
    t.data.assign(reinterpret_cast<const float*>(host_ptr), reinterpret_cast<const float*>(host_ptr) + n);
    c->host[k] = std::move(t);
    return TLD_OK;
}

int need(const ClipCore* c, const std::string& key, const std::vector<int64_t>& shape, const HostTensor** out) {
    auto it = c->host.find(key);
    if (it == c->host.end()) return fail(TLD_ERR_STATE, "missing state_dict entry '%s'", key.c_str());
    if (it->second.shape != shape) {
        std::string got, want;
        for (int64_t s : it->second.shape) got += std::to_string(s) + ",";
        for (int64_t s : shape) want += std::to_string(s) + ",";
        return fail(TLD_ERR_SHAPE, "'%s' has shape [%s], expected [%s]", key.c_str(), got.c_str(), want.c_str());
    }
    *out = &it->second;
    return TLD_OK;
}
int upload_entry(ClipCore* c, const std::string& key, const std::vector<int64_t>& shape, float** out) {
    const HostTensor* t = nullptr;
    if (int rc = need(c, key, shape, &t)) return rc;
    return upload_f32(c, t->data, out);
}
// the output projection [W, E], held transposed
int upload_proj_t(ClipCore* c, const std::string& key) {
    const int W = c->W, E = c->E;
    const HostTensor* t = nullptr;
    if (int rc = need(c, key, {W, E}, &t)) return rc;
    std::vector<float> pt((size_t)E * W);
    for (int k = 0; k < W; ++k) for (int n = 0; n < E; ++n) pt[(size_t)n * W + k] = t->data[(size_t)k * E + n];
    return upload_f32(c, pt, &c->proj_t);
}
int upload_blocks(ClipCore* c, ClipTower tower) {
    const int W = c->W;
    const HostTensor* t = nullptr;
    c->blocks.resize(c->L);
    for (int l = 0; l < c->L; ++l) {
        Block& b = c->blocks[l];
        const std::string p = clip_block_prefix(tower) + std::to_string(l) + ".";
        struct Item { const char* key; std::vector<int64_t> shape; float** f32; bf16** b16; };
        const std::vector<Item> items = {
            {"ln_1.weight", {W}, &b.ln1_g, nullptr}, {"ln_1.bias", {W}, &b.ln1_b, nullptr},
            {"attn.in_proj_weight", {3 * W, W}, nullptr, &b.in_w}, {"attn.in_proj_bias", {3 * W}, &b.in_b, nullptr},
            {"attn.out_proj.weight", {W, W}, nullptr, &b.out_w}, {"attn.out_proj.bias", {W}, &b.out_b, nullptr},
            {"ln_2.weight", {W}, &b.ln2_g, nullptr}, {"ln_2.bias", {W}, &b.ln2_b, nullptr},
            {"mlp.c_fc.weight", {4 * W, W}, nullptr, &b.fc_w}, {"mlp.c_fc.bias", {4 * W}, &b.fc_b, nullptr},
            {"mlp.c_proj.weight", {W, 4 * W}, nullptr, &b.proj_w}, {"mlp.c_proj.bias", {W}, &b.proj_b, nullptr},
        };
        for (auto& it : items) {
            if (int rc = need(c, p + it.key, it.shape, &t)) return rc;
            if (it.f32) { if (int rc = upload_f32(c, t->data, it.f32)) return rc; }
            else { if (int rc = upload_bf16(c, t->data, it.b16)) return rc; }
        }
    }
    return TLD_OK;
}

// the GEMM operands as the engine holds them, logical [N][K], read in place: named once the weights exist, whether or not the hook is on
void name_operands(ClipCore* c) {
    const int64_t W = c->W;
    c->stages.ref("proj_t", c->proj_t, ST_F32, c->E, W);
    for (int l = 0; l < (int)c->blocks.size(); ++l) {
        const Block& b = c->blocks[l];
        const std::string pre = "blk" + std::to_string(l) + ".";
        c->stages.ref(pre + "in_w", b.in_w, ST_BF16, 3 * W, W); c->stages.ref(pre + "out_w", b.out_w, ST_BF16, W, W);
        c->stages.ref(pre + "fc_w", b.fc_w, ST_BF16, 4 * W, W); c->stages.ref(pre + "proj_w", b.proj_w, ST_BF16, W, 4 * W);
    }
}
// the end of finalize_weights, after the last upload
int finish_weights(ClipCore* c) {
    c->host.clear();
    HIP_TRY(hipDeviceSynchronize());
    c->finalized = true;
    name_operands(c);
    return TLD_OK;
}

// ---- the stage hook ------------------------------------------------------------------------------------------------------------

// set_debug(0) / destroy: the snapshots go, the operand names stay
void drop_snapshots(ClipCore* c) {
    c->stages.free_all();
    c->debug = false;
    if (c->finalized) name_operands(c);
}
// memory for every stage from x0 on of max_batch samples: T rows per block stage, one row per sample for the pooled row and the output
int reserve_stages(ClipCore* c, int rows) {
    const size_t B = (size_t)c->max_batch, T = B * rows, W = c->W;
    int rc = c->stages.reserve("x0", T * W * 4);
    for (int l = 0; !rc && l < c->L; ++l) {
        const std::string pre = "blk" + std::to_string(l) + ".";
        for (const char* n : {"h1", "att", "h2"}) if (!rc) rc = c->stages.reserve(pre + n, T * W * 2);
        for (const char* n : {"attn_out", "x1", "mlp_out"}) if (!rc) rc = c->stages.reserve(pre + n, T * W * 4);
        if (!rc) rc = c->stages.reserve(pre + "qkv", T * 3 * W * 2);
        for (const char* n : {"f_pre", "f"}) if (!rc) rc = c->stages.reserve(pre + n, T * 4 * W * 2);
        if (!rc && l + 1 < c->L) rc = c->stages.reserve(pre + "x2", T * W * 4);              // the last block forms only the pooled rows
    }
    if (!rc) rc = c->stages.reserve("pooled", B * W * 4);
    if (!rc) rc = c->stages.reserve("out", B * c->E * 4);
    return rc;
}
// the start of a debug encode: not under capture, earlier snapshots forgotten, and the whole workspace of max_batch samples (with a tower's
// `extra` buffer, in allocation order) NaN in bf16 and fp32 wherever this call stores nothing.  `hook` names the tower's set_debug entry
int begin_debug_call(ClipCore* c, int rows, const char* hook, hipStream_t s, bf16* extra = nullptr, size_t extra_count = 0) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone)
        return fail(TLD_ERR_STATE, "a debug encode (%s) cannot be captured into a graph", hook);
    c->stages.begin_call();
    const size_t B = (size_t)c->max_batch, TW = B * rows * c->W;
    HIP_TRY(hipMemsetAsync(c->x, 0xFF, TW * 4, s));
    HIP_TRY(hipMemsetAsync(c->tmp, 0xFF, TW * 4, s));
    HIP_TRY(hipMemsetAsync(c->pooled, 0xFF, B * c->W * 4, s));
    if (extra) HIP_TRY(hipMemsetAsync(extra, 0xFF, extra_count * 2, s));
    HIP_TRY(hipMemsetAsync(c->h, 0xFF, TW * 2, s));
    HIP_TRY(hipMemsetAsync(c->qkv, 0xFF, TW * 3 * 2, s));
    HIP_TRY(hipMemsetAsync(c->att, 0xFF, TW * 2, s));
    HIP_TRY(hipMemsetAsync(c->f, 0xFF, TW * 4 * 2, s));
    return TLD_OK;
}
int read_stage(ClipCore* c, const char* name, float* host_out, int64_t numel, int64_t* shape4) {
    if (!c || !name || !host_out) return fail(TLD_ERR_INVALID, "null argument");
    DeviceGuard guard(c->device_id);
    return c->stages.read(name, host_out, numel, shape4);
}

int64_t weight_bytes(const ClipCore* c) { return c ? c->weight_bytes : 0; }

// destroy, but for the delete (the tower's own type)
void release(ClipCore* c) {
    DeviceGuard guard(c->device_id);
    drop_snapshots(c);
    for (void* p : c->allocs) (void)hipFree(p);
}

// ---- encode ------------------------------------------------------------------------------------------------------------------

int check_encode(const ClipCore* c, int batch) {
    if (!c->finalized) return fail(TLD_ERR_STATE, "weights not finalized");
    if (batch < 1 || batch > c->max_batch) return fail(TLD_ERR_INVALID, "batch=%d outside 1..max_batch=%d", batch, c->max_batch);
    return TLD_OK;
}

// a stage snapshot right after the launch that completed it; nothing with the hook off.  `c` and `s` are the caller's engine and stream
#define CLIP_KEEP(name, src, dtype, rows, cols) do { if (c->debug) { if (int rc_ = c->stages.copy(name, src, dtype, s, rows, cols)) return rc_; } } while (0)

// From x = the tower's embedding (fp32 [batch * n, W]): h = ln_1 of block 0, the L blocks, the pooled row of each sample (row eot[b], or row 0 when
// eot is null) through the final LayerNorm (lnf_g, lnf_b), and its fp32 projection into out [batch, E].  attention() launches the tower's kernel on
// c->qkv -> c->att.  `entry` is the tower's encode entry, for the text of a refused GEMM.
template <typename Attention>
int run_blocks(ClipCore* c, int batch, int n, Attention&& attention, const int* eot, const float* lnf_g, const float* lnf_b, const char* entry, float* out,
               hipStream_t s) {
#define GEMM(what, ...) GEMM_TRY(std::string(entry) + ", block " + std::to_string(l) + " " what, gemm(__VA_ARGS__))
    const int W = c->W, T = batch * n;
    const bool dbg = c->debug;
    const dim3 rows((T + 3) / 4);
    CLIP_KEEP("x0", c->x, ST_F32, T, W);
    hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, (const float*)nullptr, (const float*)nullptr, c->blocks[0].ln1_g, c->blocks[0].ln1_b, c->h, T, W);
    for (int l = 0; l < c->L; ++l) {
        const Block& b = c->blocks[l];
        const std::string pre = dbg ? "blk" + std::to_string(l) + "." : std::string();
        CLIP_KEEP(pre + "h1", c->h, ST_BF16, T, W);
        GEMM("in_proj", c->h, W, b.in_w, T, 3 * W, W, EPI_BIAS_BF16, b.in_b, c->qkv, nullptr, s);
        CLIP_KEEP(pre + "qkv", c->qkv, ST_BF16, T, 3 * W);
        attention();
        CLIP_KEEP(pre + "att", c->att, ST_BF16, T, W);
        GEMM("out_proj", c->att, W, b.out_w, T, W, W, EPI_F32, nullptr, nullptr, c->tmp, s);
        CLIP_KEEP(pre + "attn_out", c->tmp, ST_F32, T, W);
        hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, c->tmp, b.out_b, b.ln2_g, b.ln2_b, c->h, T, W);
        CLIP_KEEP(pre + "x1", c->x, ST_F32, T, W);
        CLIP_KEEP(pre + "h2", c->h, ST_BF16, T, W);
        GEMM("c_fc", c->h, W, b.fc_w, T, 4 * W, W, EPI_BIAS_BF16, b.fc_b, c->f, nullptr, s);
        CLIP_KEEP(pre + "f_pre", c->f, ST_BF16, T, 4 * W);
        {
            const long n8 = (long)T * 4 * W / 8;
            hipLaunchKernelGGL(clip_quickgelu_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, s, c->f, n8);
        }
        CLIP_KEEP(pre + "f", c->f, ST_BF16, T, 4 * W);
        GEMM("c_proj", c->f, 4 * W, b.proj_w, T, W, 4 * W, EPI_F32, nullptr, nullptr, c->tmp, s);
        CLIP_KEEP(pre + "mlp_out", c->tmp, ST_F32, T, W);
        if (l + 1 < c->L) {
            hipLaunchKernelGGL(clip_add_ln_kernel, rows, dim3(256), 0, s, c->x, c->tmp, b.proj_b, c->blocks[l + 1].ln1_g, c->blocks[l + 1].ln1_b, c->h, T, W);
            CLIP_KEEP(pre + "x2", c->x, ST_F32, T, W);
        } else {
            // the pooled row of each sample only: residual add of the last block + the final LayerNorm
            hipLaunchKernelGGL(clip_final_ln_kernel, dim3(batch), dim3(64), 0, s, c->x, c->tmp, b.proj_b, eot, lnf_g, lnf_b, c->pooled, W, n);
            CLIP_KEEP("pooled", c->pooled, ST_F32, batch, W);
        }
    }
    launch_linear_f32(c->pooled, W, c->proj_t, nullptr, out, c->E, batch, W, c->E, 0, s);
    CLIP_KEEP("out", out, ST_F32, batch, c->E);
#undef GEMM
    return TLD_OK;
}

}  // namespace
}  // namespace tld

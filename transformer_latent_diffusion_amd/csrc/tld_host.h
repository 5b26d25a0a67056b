// tld_host.h -- the host plumbing the four engines (tld_engine / tld_vae / tld_clip / tld_train .hip) share: status and error text, the device
// guard, bf16 conversion, device allocation and upload, and the ONE stage hook (StageStore) under tld_*_set_debug / tld_*_read_stage.
// Host-only; include after tld_common.h.
#pragma once

#include <map>
#include <string>
#include <vector>

#include "tld_stages.h"      // fail, f32_to_bf16_rne / bf16_to_f32, the stage types and decode_stage (no HIP in there)

namespace tld {

#define HIP_TRY(expr)                                                                                                            \
    do {                                                                                                                         \
        hipError_t _e = (expr);                                                                                                  \
        if (_e != hipSuccess) return fail(TLD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

// a refused GEMM plan launches nothing: the call fails with launch_gemm's text instead of going on over the previous call's buffers
#define GEMM_TRY(what, expr)                                                                                                     \
    do {                                                                                                                         \
        if (int _g = (expr)) { const std::string _m = tld_last_error(); return fail(_g, "%s: %s refused: %s", std::string(what).c_str(), #expr, _m.c_str()); } \
    } while (0)

// Every ABI entry point runs with the engine's device current and puts the caller's device back on exit: the
// library never changes the calling thread's current HIP device (a model on cuda:1 used from a thread whose
// current device is cuda:0 would otherwise silently redirect the caller's later allocations and launches).
// A thread with no current device yet gets the engine's.  (Raw-pointer debug hooks: PtrDeviceGuard, tld_common.h.)
struct DeviceGuard {
    int prev = -1; bool switched = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
        else if (prev < 0) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() { if (switched) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

inline int check_launch(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(TLD_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return TLD_OK;
}

// What an engine allocated, freed at destroy.  `pad` bytes are added to every allocation: kernels' over-read margins rest on it, so it is the
// engine's own figure (256 in the denoiser, 0 in the VAE and the text tower, where an empty tensor still gets 16 bytes).
struct DeviceArena {
    std::vector<void*> allocs;
    int64_t weight_bytes = 0;
    size_t pad = 0;
};
template <typename T>
int dev_alloc(DeviceArena* a, T** out, size_t count, bool weight = false) {
    void* p = nullptr;
    const size_t bytes = count * sizeof(T) + a->pad;
    HIP_TRY(hipMalloc(&p, bytes > 0 ? bytes : 16));
    a->allocs.push_back(p);
    if (weight) a->weight_bytes += (int64_t)(count * sizeof(T));
    *out = reinterpret_cast<T*>(p);
    return TLD_OK;
}
inline int upload_f32(DeviceArena* a, const std::vector<float>& h, float** out) {
    if (int rc = dev_alloc(a, out, h.size(), true)) return rc;
    HIP_TRY(hipMemcpy(*out, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return TLD_OK;
}
inline int upload_bf16(DeviceArena* a, const std::vector<float>& h, bf16** out) {
    std::vector<uint16_t> t(h.size());
    for (size_t i = 0; i < h.size(); ++i) t[i] = f32_to_bf16_rne(h[i]);
    if (int rc = dev_alloc(a, out, h.size(), true)) return rc;
    HIP_TRY(hipMemcpy(*out, t.data(), t.size() * 2, hipMemcpyHostToDevice));
    return TLD_OK;
}

// ---- the stage hook -----------------------------------------------------------------------------------------------------------
// A named tensor in its stored type (tld_stages.h), read in place (`ref`: the engine's own buffer) or from a copy the store owns (`reserve` +
// `copy` / `sink`).  A name is reserved or referenced, never both.  Each engine owns one store and keeps only its list of names and sizes, its
// SNAP one-liner and its poison step; whether the hook is on is the engine's flag, checked before it calls in here.
struct Stage {
    void* ptr = nullptr; const void* aux = nullptr; int dtype = ST_F32, layout = SL_PLAIN; int64_t shape[4] = {1, 1, 1, 1};
    StageExtra extra; bool owned = false; size_t cap = 0; bool live = false;
};
struct StageStore {
    std::map<std::string, Stage> stages;

    void free_all() {
        for (auto& kv : stages) if (kv.second.owned && kv.second.ptr) (void)hipFree(kv.second.ptr);
        stages.clear();
    }
    // start of a debug call: every snapshot of an earlier call is forgotten (its memory and the referenced names stay)
    void begin_call() { for (auto& kv : stages) if (kv.second.owned) kv.second.live = false; }
    // owned snapshot memory under a name; nothing happens when the name already has that much
    int reserve(const std::string& name, size_t bytes) {
        Stage& st = stages[name];
        if (st.owned && st.cap >= bytes) return TLD_OK;
        if (st.owned && st.ptr) (void)hipFree(st.ptr);
        st = Stage();
        if (hipMalloc(&st.ptr, bytes) != hipSuccess) {
            st.ptr = nullptr; (void)hipGetLastError();
            return fail(TLD_ERR_HIP, "stage hook: hipMalloc of %zu bytes for the snapshot '%s' failed", bytes, name.c_str());
        }
        st.owned = true; st.cap = bytes;
        return TLD_OK;
    }
    // the engine's own buffer under a name (nothing is copied)
    Stage* ref(const std::string& name, const void* ptr, int dtype, int64_t s0, int64_t s1 = 1, int64_t s2 = 1, int64_t s3 = 1, int64_t outer_stride = 0,
               int layout = SL_PLAIN) {
        if (!ptr) return nullptr;
        Stage* st = slot(name, dtype, layout, s0, s1, s2, s3);
        st->owned = false; st->ptr = const_cast<void*>(ptr); st->extra.outer_stride = outer_stride;
        return st;
    }
    // a device-to-device copy on the stream, right after the kernel that completed the value, into reserved memory.  grow: the memory is
    // reserved here when the name has none or too little (the VAE, whose stage sizes follow the call's resolution)
    int copy(const std::string& name, const void* src, int dtype, hipStream_t s, int64_t s0, int64_t s1 = 1, int64_t s2 = 1, int64_t s3 = 1,
             int layout = SL_PLAIN, bool grow = false) {
        const size_t bytes = (size_t)(s0 * s1 * s2 * s3) * st_bytes(dtype);
        if (grow) { if (int rc = reserve(name, bytes)) return rc; }
        auto it = stages.find(name);
        if (it == stages.end() || !it->second.owned || it->second.cap < bytes)
            return fail(TLD_ERR_STATE, "stage hook: no snapshot memory reserved for '%s' (%zu bytes): set_debug(1) reserves it, after the engine's mode is chosen",
                        name.c_str(), bytes);
        slot(name, dtype, layout, s0, s1, s2, s3);
        HIP_TRY(hipMemcpyAsync(it->second.ptr, src, bytes, hipMemcpyDeviceToDevice, s));
        return TLD_OK;
    }
    // a snapshot a kernel writes itself: *out is the reserved memory for fp32 [rows, cols]
    int sink(const std::string& name, int64_t rows, int64_t cols, float** out) {
        *out = nullptr;
        auto it = stages.find(name);
        if (it == stages.end() || !it->second.owned || it->second.cap < (size_t)(rows * cols) * 4)
            return fail(TLD_ERR_STATE, "stage hook: no snapshot memory reserved for '%s' (%zu bytes)", name.c_str(), (size_t)(rows * cols) * 4);
        slot(name, ST_F32, SL_PLAIN, rows, cols, 1, 1);
        *out = static_cast<float*>(it->second.ptr);
        return TLD_OK;
    }
    const Stage* find(const std::string& name) const {
        auto it = stages.find(name);
        return (it != stages.end() && it->second.live && it->second.ptr) ? &it->second : nullptr;
    }
    // shape4 (may be null) receives the logical shape whenever the stage exists; host_out (may be null: shape only) fp32 [numel].  Synchronises the device.
    int read(const std::string& name, float* host_out, int64_t numel, int64_t* shape4) const {
        const Stage* st = find(name);
        if (!st) return fail(TLD_ERR_KEY, "no captured stage named '%s' (was debug enabled before the call? a stage of another path?)", name.c_str());
        if (shape4) for (int i = 0; i < 4; ++i) shape4[i] = st->shape[i];
        if (!host_out) return TLD_OK;
        const int64_t n = stage_numel(st->shape), stride = st->extra.outer_stride;
        if (numel != n)
            return fail(TLD_ERR_SHAPE, "stage '%s' has %lld elements [%lld, %lld, %lld, %lld], the caller's buffer %lld", name.c_str(), (long long)n,
                        (long long)st->shape[0], (long long)st->shape[1], (long long)st->shape[2], (long long)st->shape[3], (long long)numel);
        HIP_TRY(hipDeviceSynchronize());
        const size_t esz = st_bytes(st->dtype);
        const int64_t outer = stride ? st->shape[0] : 1, inner = stride ? n / (outer ? outer : 1) : n;
        std::vector<uint8_t> raw((size_t)((outer ? outer - 1 : 0) * stride + inner) * esz), sc;
        for (int64_t o = 0; o < outer; ++o)       // the runs land at the device's own offsets: decode_stage undoes the pitch
            HIP_TRY(hipMemcpy(raw.data() + (size_t)(o * stride) * esz, static_cast<const char*>(st->ptr) + (size_t)(o * stride) * esz, (size_t)inner * esz, hipMemcpyDeviceToHost));
        if (st->dtype == ST_MX8W) {
            sc.resize((size_t)(n / 32));
            HIP_TRY(hipMemcpy(sc.data(), st->aux, sc.size(), hipMemcpyDeviceToHost));
        }
        return decode_stage(raw.data(), sc.data(), st->dtype, st->layout, st->shape, st->extra, host_out);
    }

private:
    Stage* slot(const std::string& name, int dtype, int layout, int64_t s0, int64_t s1, int64_t s2, int64_t s3) {
        Stage& st = stages[name];
        st.dtype = dtype; st.layout = layout; st.shape[0] = s0; st.shape[1] = s1; st.shape[2] = s2; st.shape[3] = s3; st.live = true;
        return &st;
    }
};

}  // namespace tld

// tld_stages.h -- how a stage of the stage hook is stored, and the pure host function that turns the stored bytes into logical fp32.
// No HIP in this file: tests/host/stage_decode_main.cpp compiles it on its own, and tld_debug_decode_stage hands it to the CPU suite.
// The store that fills and reads stages on the device is StageStore in tld_host.h.
#pragma once

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../include/tld_hip.h"

namespace tld {

void set_last_error(const char* msg);      // thread-local message behind tld_last_error() (tld_engine.hip)

inline int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    set_last_error(buf);
    return code;
}

inline uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);   // NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
inline float bf16_to_f32(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// Stored type.  ST_U8 = raw bytes (the e4m3 codes of an fp8 A operand); ST_MX8S = E8M0 scale bytes stored [cols / 4][rows][4], logical [rows, cols];
// ST_MX8W = an e4m3 weight [rows, cols] with its scales (`aux`, [cols / 128][rows][4]), dequantised here
enum { ST_F32 = TLD_STAGE_F32, ST_BF16 = TLD_STAGE_BF16, ST_U8 = TLD_STAGE_U8, ST_MX8S = TLD_STAGE_MX8S, ST_MX8W = TLD_STAGE_MX8W };
inline size_t st_bytes(int dtype) { return dtype == ST_F32 ? 4 : dtype == ST_BF16 ? 2 : 1; }
// Stored order.  SL_QKV_ROWS = shape[0] = 3 d rows in the fused QKV -> attention kernel's [head][feature half][q | k | v][32] order (logical: [q; k; v] x
// [head][64]); SL_NHWC = logical shape (B, C, H, W) stored [B][H][W][C]
enum { SL_PLAIN = TLD_STAGE_PLAIN, SL_QKV_ROWS = TLD_STAGE_QKV_ROWS, SL_NHWC = TLD_STAGE_NHWC };
struct StageExtra {
    int64_t outer_stride = 0;       // != 0: shape[0] runs of shape[1..3] elements, `outer_stride` elements apart (tables with a per-layer pitch)
    int d = 0, heads = 0;           // SL_QKV_ROWS only: the model width and head count (d = 64 heads)
};
inline int64_t stage_numel(const int64_t* s) { return s[0] * s[1] * s[2] * s[3]; }

// raw (and aux_raw for ST_MX8W) as the device holds them -> out: stage_numel(shape4) logical fp32 values.  Every conversion is exact.
inline int decode_stage(const void* raw, const void* aux_raw, int dtype, int layout, const int64_t* shape4, const StageExtra& x, float* out) {
    if (!raw || !shape4 || !out || (dtype == ST_MX8W && !aux_raw)) return fail(TLD_ERR_INVALID, "decode_stage: null argument");
    for (int i = 0; i < 4; ++i) if (shape4[i] < 0) return fail(TLD_ERR_INVALID, "decode_stage: negative dimension");
    const int64_t n = stage_numel(shape4);
    const uint8_t* bytes = static_cast<const uint8_t*>(raw);
    if (dtype == ST_U8 || dtype == ST_MX8S || dtype == ST_MX8W) {
        const int64_t rows = shape4[0], cols = shape4[1];
        if (layout != SL_PLAIN || x.outer_stride || rows * cols != n || (dtype == ST_MX8S && cols % 4) || (dtype == ST_MX8W && cols % 128))
            return fail(TLD_ERR_INVALID, "decode_stage: byte stages are plain [rows, columns] (columns a multiple of 4 for scales, of 128 for fp8 weights)");
        const uint8_t* sc = static_cast<const uint8_t*>(aux_raw);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t c = 0; c < cols; ++c) {
                float v;
                if (dtype == ST_U8) v = (float)bytes[r * cols + c];
                else if (dtype == ST_MX8S) v = (float)bytes[((c >> 2) * rows + r) * 4 + (c & 3)];
                else {                          // e4m3 code x 2^(E8M0 - 127)   (the quantiser saturates: no NaN code is stored)
                    const uint8_t q = bytes[r * cols + c];
                    const int ex = (q >> 3) & 15, man = q & 7;
                    const float mag = ex ? ldexpf((float)(8 + man), ex - 10) : ldexpf((float)man, -9);
                    v = ldexpf((q & 0x80) ? -mag : mag, (int)sc[((c >> 7) * rows + r) * 4 + ((c >> 5) & 3)] - 127);
                }
                out[r * cols + c] = v;
            }
        return TLD_OK;
    }
    if (dtype != ST_F32 && dtype != ST_BF16) return fail(TLD_ERR_INVALID, "decode_stage: unknown dtype %d", dtype);
    auto load = [&](int64_t i) {
        if (dtype == ST_BF16) { uint16_t h; memcpy(&h, bytes + i * 2, 2); return bf16_to_f32(h); }
        float f; memcpy(&f, bytes + i * 4, 4); return f;
    };
    const int64_t outer = x.outer_stride ? shape4[0] : 1, inner = x.outer_stride ? shape4[1] * shape4[2] * shape4[3] : n, pitch = x.outer_stride ? x.outer_stride : inner;
    if (layout == SL_PLAIN) {
        for (int64_t o = 0; o < outer; ++o)
            for (int64_t i = 0; i < inner; ++i) out[o * inner + i] = load(o * pitch + i);
    } else if (layout == SL_NHWC && !x.outer_stride) {
        const int64_t B = shape4[0], C = shape4[1], HW = shape4[2] * shape4[3];
        for (int64_t b = 0; b < B; ++b)
            for (int64_t p = 0; p < HW; ++p)
                for (int64_t c = 0; c < C; ++c) out[(b * C + c) * HW + p] = load((b * HW + p) * C + c);
    } else if (layout == SL_QKV_ROWS && !x.outer_stride) {      // the inverse of the packing in refresh_fold_kernel
        const int64_t d = x.d, row = shape4[0] ? n / shape4[0] : 0;
        if (d <= 0 || d != (int64_t)x.heads * 64 || shape4[0] != 3 * d) return fail(TLD_ERR_INVALID, "decode_stage: packed QKV rows need shape[0] = 3 d and d = 64 heads");
        for (int64_t h = 0; h < x.heads; ++h)
            for (int part = 0; part < 3; ++part)
                for (int64_t c = 0; c < 64; ++c) {
                    const int64_t logical = part * d + h * 64 + c, packed = h * 192 + (c >> 5) * 96 + part * 32 + (c & 31);
                    for (int64_t j = 0; j < row; ++j) out[logical * row + j] = load(packed * row + j);
                }
    } else {
        return fail(TLD_ERR_INVALID, "decode_stage: layout %d (with an outer stride: plain only)", layout);
    }
    return TLD_OK;
}

}  // namespace tld

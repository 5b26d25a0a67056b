// Stand-alone driver of decode_stage (csrc/tld_stages.h) for a sanitizer build: the cases of tests/test_stage_decode_host.py on heap buffers of exactly
// the stored size, so that a read or write past either end is caught.  No HIP, no Python:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all tests/host/stage_decode_main.cpp -o stage_decode_main && ./stage_decode_main
#include <cstdlib>
#include <string>
#include <vector>

#include "../../transformer_latent_diffusion_amd/csrc/tld_stages.h"

namespace tld {
static std::string g_last;
void set_last_error(const char* msg) { g_last = msg; }
}  // namespace tld
using namespace tld;

static int g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_bad; } } while (0)

static bool same_bits(const std::vector<float>& a, const std::vector<float>& b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * 4); }
static std::vector<uint16_t> halves(size_t n, uint32_t seed) {
    std::vector<uint16_t> h(n);
    for (auto& v : h) { seed = seed * 1664525u + 1013904223u; v = (uint16_t)(seed >> 13); }
    return h;
}

int main() {
    {   // bf16 plain: +-0, NaN patterns, the largest finite value
        const std::vector<uint16_t> h = {0x0000, 0x8000, 0x7FC1, 0xFFFF, 0x7F7F, 0xFF7F, 0x0001, 0x3F80, 0xC2F7, 0x7F80};
        const int64_t sh[4] = {2, 5, 1, 1};
        std::vector<float> out(10), want(10);
        for (size_t i = 0; i < 10; ++i) want[i] = bf16_to_f32(h[i]);
        CHECK(decode_stage(h.data(), nullptr, ST_BF16, SL_PLAIN, sh, StageExtra(), out.data()) == TLD_OK && same_bits(out, want));
    }
    {   // bytes, and the [cols / 4][rows][4] scale layout at rows = 3, cols = 8
        std::vector<uint8_t> b(24);
        for (size_t i = 0; i < b.size(); ++i) b[i] = (uint8_t)(250 - 7 * i);
        const int64_t sh[4] = {3, 8, 1, 1};
        std::vector<float> out(24), want(24);
        for (size_t i = 0; i < 24; ++i) want[i] = (float)b[i];
        CHECK(decode_stage(b.data(), nullptr, ST_U8, SL_PLAIN, sh, StageExtra(), out.data()) == TLD_OK && same_bits(out, want));
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 8; ++c) want[r * 8 + c] = (float)b[((c / 4) * 3 + r) * 4 + c % 4];
        CHECK(decode_stage(b.data(), nullptr, ST_MX8S, SL_PLAIN, sh, StageExtra(), out.data()) == TLD_OK && same_bits(out, want));
    }
    {   // fp8 weights at rows = 2, cols = 128: every e4m3 code, scales 127, 0 and others
        std::vector<uint8_t> q(256), sc = {127, 0, 130, 120, 97, 127, 0, 140};
        for (int i = 0; i < 256; ++i) q[i] = (uint8_t)(i * 37 + 11);       // a permutation of 0 ... 255
        const int64_t sh[4] = {2, 128, 1, 1};
        std::vector<float> out(256), want(256);
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 128; ++c) {
                const int code = q[r * 128 + c], ex = (code >> 3) & 15, man = code & 7;
                const double mag = ex ? (8 + man) * ldexp(1.0, ex - 10) : man * ldexp(1.0, -9);
                want[r * 128 + c] = (float)ldexp((code & 0x80) ? -mag : mag, (int)sc[r * 4 + c / 32] - 127);
            }
        CHECK(decode_stage(q.data(), sc.data(), ST_MX8W, SL_PLAIN, sh, StageExtra(), out.data()) == TLD_OK && same_bits(out, want));
        CHECK(decode_stage(q.data(), nullptr, ST_MX8W, SL_PLAIN, sh, StageExtra(), out.data()) == TLD_ERR_INVALID && !g_last.empty());
    }
    {   // NHWC at B = 2, C = 3, H = 2, W = 2
        const std::vector<uint16_t> h = halves(24, 3);
        const int64_t sh[4] = {2, 3, 2, 2};
        std::vector<float> out(24), want(24);
        for (int b = 0; b < 2; ++b) for (int c = 0; c < 3; ++c) for (int p = 0; p < 4; ++p) want[(b * 3 + c) * 4 + p] = bf16_to_f32(h[(b * 4 + p) * 3 + c]);
        CHECK(decode_stage(h.data(), nullptr, ST_BF16, SL_NHWC, sh, StageExtra(), out.data()) == TLD_OK && same_bits(out, want));
    }
    {   // packed QKV rows at d = 128, 2 heads, row length 2
        std::vector<float> packed(384 * 2), out(384 * 2), want(384 * 2);
        for (size_t i = 0; i < packed.size(); ++i) packed[i] = (float)i * 0.25f - 50.0f;
        for (int h = 0; h < 2; ++h) for (int part = 0; part < 3; ++part) for (int c = 0; c < 64; ++c)
            for (int j = 0; j < 2; ++j) want[(part * 128 + h * 64 + c) * 2 + j] = packed[(h * 192 + (c / 32) * 96 + part * 32 + c % 32) * 2 + j];
        const int64_t sh[4] = {384, 2, 1, 1};
        StageExtra x; x.d = 128; x.heads = 2;
        CHECK(decode_stage(packed.data(), nullptr, ST_F32, SL_QKV_ROWS, sh, x, out.data()) == TLD_OK && same_bits(out, want));
        x.heads = 3;
        CHECK(decode_stage(packed.data(), nullptr, ST_F32, SL_QKV_ROWS, sh, x, out.data()) == TLD_ERR_INVALID);
    }
    {   // an outer stride of 20 over runs of 12, shape (2, 3, 4, 1): the stored span is 32 elements
        const std::vector<uint16_t> h = halves(32, 7);
        const int64_t sh[4] = {2, 3, 4, 1};
        std::vector<float> out(24), want(24);
        for (int o = 0; o < 2; ++o) for (int i = 0; i < 12; ++i) want[o * 12 + i] = bf16_to_f32(h[o * 20 + i]);
        StageExtra x; x.outer_stride = 20;
        CHECK(decode_stage(h.data(), nullptr, ST_BF16, SL_PLAIN, sh, x, out.data()) == TLD_OK && same_bits(out, want));
        CHECK(decode_stage(h.data(), nullptr, ST_BF16, SL_NHWC, sh, x, out.data()) == TLD_ERR_INVALID);
    }
    {   // null pointers
        const int64_t sh[4] = {1, 1, 1, 1};
        float one = 0.f;
        g_last.clear();
        CHECK(decode_stage(nullptr, nullptr, ST_F32, SL_PLAIN, sh, StageExtra(), &one) == TLD_ERR_INVALID && !g_last.empty());
        CHECK(decode_stage(&one, nullptr, ST_F32, SL_PLAIN, sh, StageExtra(), nullptr) == TLD_ERR_INVALID);
        CHECK(decode_stage(&one, nullptr, 9, SL_PLAIN, sh, StageExtra(), &one) == TLD_ERR_INVALID);
    }
    printf(g_bad ? "stage_decode_main: %d checks FAILED\n" : "stage_decode_main: all checks passed\n", g_bad);
    return g_bad ? EXIT_FAILURE : EXIT_SUCCESS;
}

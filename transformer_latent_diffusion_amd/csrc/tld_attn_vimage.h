// tld_attn_vimage.h -- the LDS image of V that the fused QKV + attention epilogues write and attn256_wave (tld_attn_core.h) reads.  Plain C++, no HIP
// types: the kernels and tests/host/attn_vimage_main.cpp compile the same functions.
//
// V is ROW-major, [256 keys][64 features] bf16 in 128-byte rows with no pad (32 KiB), written like the K and Q images: one 8-byte store per register quad
// (4 consecutive features of the lane's token).  The A operand of O^T = V^T P^T -- 8 keys of ONE feature per lane -- comes out of it with gfx950's
// transposing LDS read (ds_read_b64_tr_b16), two reads per fragment.  Per group of 16 lanes that instruction gathers a block of 4 rows x 16 columns of
// 16-bit elements: lane 4q + p of the group supplies the address of row q, columns 4p .. 4p + 3; lane i receives column i, row q in element q.
//
// Swizzle.  A 32-lane half of one read covers keys k0 .. k0 + 3 (k0 % 4 == 0) x 32 features = 4 rows x 64 bytes, and a 128-byte row spans 32 of the 64
// banks the read is served from ((addr / 4) % 64 per half): rows k0 and k0 + 2 start in the same bank, so their 64 bytes must sit in different halves
// of the row.  The K / Q swizzle chunk ^ ((row >> 1) & 7) moves rows k0 and k0 + 2 by 1 within the same half (2-way conflicts); here bit 2 of the chunk
// is flipped by row bit 1, and the low two bits by row bits 2 and 0 so that the 8-byte WRITES of 32 consecutive rows (lane = row, one chunk) spread over
// all eight chunk positions, four rows each -- the floor for 512 bytes through 32 banks, and what the K / Q writes have.  No row bit above 2 takes part:
// the key step and the second read of a fragment (rows + 16, + 8) are constants added to a lane's address, immediates of the instruction.
#pragma once

namespace tld {

constexpr int kAttnVRowBytes = 128;                       // 64 features x bf16
constexpr int kAttnVImageBytes = 256 * kAttnVRowBytes;    // 256 keys

constexpr int attn_v_swizzle(int row) { return (((row >> 1) & 1) << 2) | (((row >> 2) & 1) << 1) | (row & 1); }

// byte offset of features f .. f + 3 (f % 4 == 0) of key `row`: the store address of one register quad, and what every read address is made of
constexpr int attn_v_off(int row, int f) { return row * kAttnVRowBytes + ((((f >> 3) ^ attn_v_swizzle(row)) << 4) | ((f & 7) << 1)); }

// The address lane `lane` (0 .. 63) supplies to transposed read rd (0, 1) of the fragment of PV step s2 (0 .. 15: keys 16 s2 ..) and feature tile ct (0, 1).
// The lane (l31 = lane & 31, hi = lane >> 5) receives feature 32 ct + l31 of keys 16 s2 + 8 rd + 4 hi + {0 .. 3}: elements 4 rd .. 4 rd + 3 of the MFMA's
// A operand, the key order of the P operand.  Its group of 16 is features 32 ct + 16 g ..; it addresses row q = (lane >> 2) & 3 of the block, columns 4p ..
constexpr int attn_v_tr_addr(int lane, int s2, int ct, int rd) {
    const int hi = lane >> 5, g = (lane >> 4) & 1, q = (lane >> 2) & 3, p = lane & 3;
    return attn_v_off(16 * s2 + 8 * rd + 4 * hi + q, 32 * ct + 16 * g + 4 * p);
}

// The same address from the lane's one base attn_v_tr_addr(lane, 0, 0, 0): s2 and rd never reach the swizzle (constants, 2 KiB per step and 1 KiB for the
// second read), ct flips chunk bit 2 = address bit 6 whatever the lane (the sign of the change is lane dependent, the flipped bit is not).  This is the
// form attn256_wave uses: one base register, one v_xor for the second feature tile.
constexpr int attn_v_tr_step(int base, int s2, int ct, int rd) { return (base ^ (ct * 64)) + (16 * s2 + 8 * rd) * kAttnVRowBytes; }

namespace vimage_detail {
constexpr bool tr_step_is_tr_addr() {
    for (int lane = 0; lane < 64; ++lane)
        for (int s2 = 0; s2 < 16; ++s2)
            for (int ct = 0; ct < 2; ++ct)
                for (int rd = 0; rd < 2; ++rd)
                    if (attn_v_tr_step(attn_v_tr_addr(lane, 0, 0, 0), s2, ct, rd) != attn_v_tr_addr(lane, s2, ct, rd)) return false;
    return true;
}
}  // namespace vimage_detail
static_assert(vimage_detail::tr_step_is_tr_addr(), "attn_v_tr_step must reproduce attn_v_tr_addr for every lane, step, feature tile and read");

// ---- LDS map of the two-head epilogue (EPI_QKV_ATTN2, tld_gemm.hip): five 32-KiB images are the CU's 160 KiB to the byte ------------------------------------
// Phase 1, until the barrier behind the LayerNorm-1 correction: the side tables (row partial sums | (mean, rstd) | c1, b1 of the tile's 384 columns) lie at
// [0, kPairTabBytes) and are still read, while the corrected accumulators already go to K_A, V_A, Q (head A's q) and K_B.  Phase 2, behind that barrier:
// V_B overlays the tables; Q is rewritten with head B's q between the two heads.  Nothing else fits: head B's q waits in the workgroup's global slot.
constexpr int kPairLdsBytes = 160 * 1024;
constexpr int kPairTabBytes = 256 * 8 * 8 + 256 * 8 + 2 * 384 * 4;
constexpr int kPairImgBytes = 256 * 128;
constexpr int kPairVB = 0, kPairKA = 1 * kPairImgBytes, kPairVA = 2 * kPairImgBytes, kPairQ = 3 * kPairImgBytes, kPairKB = 4 * kPairImgBytes;
struct PairRegion { const char* name; int begin, end; };
constexpr PairRegion kPairPhase1[] = {{"tables", 0, kPairTabBytes},          {"K_A", kPairKA, kPairKA + kPairImgBytes}, {"V_A", kPairVA, kPairVA + kAttnVImageBytes},
                                      {"Q", kPairQ, kPairQ + kPairImgBytes}, {"K_B", kPairKB, kPairKB + kPairImgBytes}};
constexpr PairRegion kPairPhase2[] = {{"V_B", kPairVB, kPairVB + kAttnVImageBytes}, {"K_A", kPairKA, kPairKA + kPairImgBytes}, {"V_A", kPairVA, kPairVA + kAttnVImageBytes},
                                      {"Q", kPairQ, kPairQ + kPairImgBytes},        {"K_B", kPairKB, kPairKB + kPairImgBytes}};
template <int N>
constexpr bool pair_regions_ok(const PairRegion (&r)[N]) {
    for (int a = 0; a < N; ++a) {
        if (r[a].begin < 0 || r[a].end <= r[a].begin || r[a].end > kPairLdsBytes) return false;
        for (int b = a + 1; b < N; ++b)
            if (r[a].begin < r[b].end && r[b].begin < r[a].end) return false;
    }
    return true;
}
static_assert(5 * kPairImgBytes <= 163840, "five images are all of a CU's LDS");
static_assert(pair_regions_ok(kPairPhase1), "no image written before the post-correction barrier may overlap the tables (or another image)");
static_assert(pair_regions_ok(kPairPhase2), "the five images of the attention phase are disjoint and inside LDS");

}  // namespace tld

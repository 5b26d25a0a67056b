// tld_qkv_pair_plan.h -- which form of the fused QKV + attention kernel a launch gets.  Part of the kernel selection beside tld_gemm_plan.h and, like it,
// host-only integer arithmetic: no HIP, no environment, no state, and no type of the device code (tld_gemm_plan.h needs bf16 for GemmParams), so that tests/host/qkv_pair_main.cpp compiles it with any host
// compiler.  tld_debug_qkv_pair_plan (include/tld_hip.h) exposes it; the engine's run_body asks it per launch.
#pragma once

namespace tld {

// ---- fused QKV + attention: one head per 256 x 192 tile (EPI_QKV_ATTN) or two per 256 x 384 tile (EPI_QKV_ATTN2) ---------------------------------------------------
// The two forms give the same bits (tests/test_gpu_qkv_pair.py), so the choice may follow the batch size.  Every workgroup walks ceil(tiles / CUs) tiles, so the pair
// form is taken where  ceil(pairs / CUs) t_pair < ceil(items / CUs) t_item  with items = samples x heads, pairs = items / 2.  t_pair / t_item = kQkvPairCostNum /
// kQkvPairCostDen comes from the two kernels' time per launch at C1's block size (128 samples x 12 heads: 768 pairs in 3 whole rounds, 1536 items in 6, on 256 CUs):
// 138.4 us against 148.3 us, t_pair / t_item = 1.87 - 1.90, while all of the second head waited in the global slot (profiles/qkv_pair_ab.txt); with its k and v
// resident in LDS and the row-major V image in both kernels, under HIP events and with block 0's launch taken as half a full one: t_item = 141.85 x 12 / 11.5 =
// 148.0 us, t_pair = (125.3 x 12 - 74.0) / 11 = 130.0 us, t_pair / t_item = 2 x 130.0 / 148.0 = 1.76 (profiles/qkv_resident_ab.txt); rounded up to 1.8.
// At C1 blocks 1 - 11 take pairs; block 0 on the shared half batch (64 x 12: 1.5 rounds of pairs against 3 whole rounds of items) and small batches keep
// the one-head kernel.
constexpr long kQkvPairCostNum = 18, kQkvPairCostDen = 10;
inline bool plan_qkv_pair(long samples, long heads, long cus) {
    if (samples < 1 || heads < 2 || heads % 2 != 0 || cus < 1) return false;
    const long items = samples * heads, pairs = items / 2;
    const long rounds_pair = (pairs + cus - 1) / cus, rounds_item = (items + cus - 1) / cus;
    return rounds_pair * kQkvPairCostNum < rounds_item * kQkvPairCostDen;
}

}  // namespace tld

"""CPU: the float64 stage references of the inference forward (tests/infer_stage_refs.py) against the reference fixtures.

The GPU stage test compares the engine with these functions, so they are held here first, chained with the fp32 weights in float64:
  * against every stage array and x0 of g1_tiny32_forward.npz and against x0 of g5_100m.npz (fp32 runs of the reference model), at the
    accuracy of an fp32 reference: |chain - fixture| <= 1e-4 max|fixture| per element.  Measured on the host: g1 stages 1.9e-7 (tokens0) ... 6.8e-5
    (tokens_final), g1 x0 4.5e-5, g5 x0 7.6e-6 (the fixtures are fp32 runs: their own rounding is what is measured);
  * cross_row's folded tables against the plain LayerNorm-2 / q / k | v statement of the same cross-attention (1e-9: both float64);
  * the update functions against the g2 sampler traces: xt[i + 1] from xt[i], x0[i], x0[i - 1] and schedule.step_coefficients, DPM-Solver++(2M)
    and DDIM, and the CFG-free final prediction's shifts (fp32 traces: 2e-5 max|xt|; measured <= 1.4e-7);
  * the kernels' rounding models against their exact statements, at the size their comments give (the degree-6 GELU polynomial within 1.7e-4
    absolute, tld_common.h; bf16 probabilities within 2^-8 relative);
  * the MX-fp8 statements of the fp8 stage test (mx8_quantize, mx8_dequantize: integer arithmetic, any device) bit for bit against
    tests/mx8_emulation.py (torch.float8_e4m3fn) on bf16 data of wide spread with zero blocks, negative zeros, ties, subnormals and saturation, and
    against the library's host quantiser; mx8_linear against the plain product of the g5 chain's operands; the difference report and the tile mask.
"""
import math

import numpy as np
import torch

import infer_stage_refs as F
import mx8_emulation as E
import train_stage_refs as R
from conftest import cfg_from_arr, load_golden, synth_weights
from transformer_latent_diffusion_amd import schedule

FP32_REF_TOL = 1e-4


def _w64(g):
    cfg = cfg_from_arr(g["cfg"])
    sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
    return cfg, {k: torch.from_numpy(np.array(v)).double() for k, v in sd.items()}


def _close(name, got, ref, tol=FP32_REF_TOL):
    ref = torch.as_tensor(ref).double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f"{name:24s} max|chain - fixture| / max|fixture| = {err:.2e}")
    assert err <= tol, (name, err)


def test_chain_reproduces_g1_stages_and_output():
    g = load_golden("g1_tiny32_forward.npz")
    cfg, w = _w64(g)
    x0, st = F.chain(cfg, w, *(torch.from_numpy(g[k]).double() for k in ("x", "sigma", "label")))
    for k in ("cond_y", "tokens0", "blk0_sa", "blk0_ca", "blk0_mlp", "tokens_final"):
        _close(k, st[k], g[k])
    _close("x0", x0, g["x0"])
    # the folded conditioning tables say the same as the plain LayerNorm-2 -> q, k | v -> softmax over two tokens
    _close("tables vs plain", st["blk0_ca"], st["blk0_ca_plain"], 1e-9)


def test_chain_reproduces_g5_output():
    g = load_golden("g5_100m.npz")
    cfg, w = _w64(g)
    x0, _ = F.chain(cfg, w, *(torch.from_numpy(g[k]).double() for k in ("x", "sigma", "label")))
    _close("g5 x0", x0, g["x0"])


def test_updates_reproduce_g2_traces():
    g = load_golden("g2_tiny32_sampler.npz")
    levels = [float(v) for v in g["noise_levels"]]
    for tag, plus in (("dpm", True), ("ddim", False)):
        co = schedule.step_coefficients(levels, plus).astype(np.float64)
        xt, x0 = torch.from_numpy(g[tag + "_xt"]).double(), torch.from_numpy(g[tag + "_x0"]).double()
        n = len(levels)
        assert xt.shape[0] == n and x0.shape[0] == n          # xt[i]: the state entering forward i; x0[i]: its CFG-combined prediction
        assert torch.equal(xt[0], torch.from_numpy(g["seeds"]).double())
        for i in range(n - 1):
            nxt = F.update(xt[i], x0[i], x0[i - 1] if i else torch.zeros_like(x0[0]), co[i])
            _close(f"{tag} xt[{i + 1}]", nxt, xt[i + 1], 2e-5)
        _close(tag + " latent", F.final_x0(x0[n - 1], float(g["sharp_f"]), float(g["bright_f"])), g[tag + "_latent"], 2e-5)


def test_masked_update_and_start_mix_are_exact_at_the_mask_ends():
    gen = torch.Generator().manual_seed(5)
    xt, x0, xp, eps, z0 = (torch.randn(2, 4, 8, 8, generator=gen, dtype=torch.float64) for _ in range(5))
    co = schedule.step_coefficients([0.9, 0.5, 0.2], True).astype(np.float64)[1]
    free = F.update(xt, x0, xp, co)
    m = torch.zeros(2, 1, 8, 8, dtype=torch.float64); m[:, :, :4] = 1.0; m[:, :, 4, :] = 0.25
    got = F.update_from(xt, x0, xp, co, 0.2, eps, z0, m)
    known = 0.2 * eps + 0.8 * z0
    assert torch.equal(got[:, :, :4], free[:, :, :4]) and torch.equal(got[:, :, 5:], known[:, :, 5:])
    assert torch.allclose(got[:, :, 4], 0.25 * free[:, :, 4] + 0.75 * known[:, :, 4], rtol=0, atol=1e-15)
    assert torch.equal(F.update_from(xt, x0, xp, co, 0.2, eps, z0, None), free)
    assert torch.equal(F.start_mix(eps, z0, 1.0), eps)
    cfg = F.cfg_combine(torch.cat([x0, xp]), 3.0)
    assert torch.allclose(cfg, xp + 3.0 * (x0 - xp), rtol=0, atol=1e-14)


def test_statistics_forms_agree():
    gen = torch.Generator().manual_seed(6)
    x = F.bf16(torch.randn(32, 768, generator=gen, dtype=torch.float64) + 0.3)
    ref = F.row_stats(x)
    for first, slots in ((True, 2), (False, 8)):
        ps = F.partial_sums(x, slots, first)
        assert ps.shape == (32, slots, 2)
        m, r = F.stats_from_sums(ps, 768)
        assert torch.allclose(torch.cat([m, r], -1), ref, rtol=1e-10, atol=1e-12)
    gamma, beta = torch.randn(768, generator=gen, dtype=torch.float64), torch.randn(768, generator=gen, dtype=torch.float64)
    W, b = torch.randn(96, 768, generator=gen, dtype=torch.float64) * 0.05, torch.randn(96, generator=gen, dtype=torch.float64)
    wf = gamma * W
    got = F.folded_linear(x, wf, wf.sum(-1), beta @ W.T + b, ref[:, :1], ref[:, 1:])
    assert torch.allclose(got, R.linear_fwd(R.ln_fwd(x, gamma, beta)[0], W, b), rtol=1e-9, atol=1e-10)


def test_rounding_models_stay_within_their_documented_size():
    y = torch.linspace(-4.0, 4.0, 20001, dtype=torch.float64)
    assert float((F.gelu_poly_half(y) - R.gelu(2 * y)).abs().max()) <= 1.7e-4          # tld_common.h: |GELU error| <= 1.7e-4 everywhere
    gen = torch.Generator().manual_seed(7)
    q, k, v = (F.bf16(torch.randn(2, 64, 128, generator=gen, dtype=torch.float64)) for _ in range(3))
    exact, model = R.attn_fwd(q, k, v, 2), F.attn_model(q, k, v, 2)
    rel = float(((model - exact) ** 2).sum().sqrt() / (exact ** 2).sum().sqrt())
    assert 0 < rel <= 2.0 ** -8, rel
    h = F.bf16(torch.randn(1, 64, 64, generator=gen, dtype=torch.float64))
    dw, db = torch.randn(64, 9, generator=gen, dtype=torch.float64) * 0.3, torch.randn(64, generator=gen, dtype=torch.float64) * 0.1
    exact = F.dw_gelu(h, dw, db, 8)
    for taps in (False, True):
        model = F.dw_gelu_model(h, dw, db, 8, taps)
        assert float((model - exact).abs().max()) <= 1.7e-4 + (2.0 ** -8 * 9 * 0.3 * 4 if taps else 0.0)


def _mx8_inputs():
    gen = torch.Generator().manual_seed(8)
    x = (torch.randn(96, 768, generator=gen) * torch.exp(torch.randn(96, 24, generator=gen) * 3).repeat_interleave(32, 1)).bfloat16().float()
    x[0, :64] = 0                                          # all-zero blocks
    x[1, 3] = -0.0; x[1, 40:48] = -0.0                     # negative zeros keep their sign bit
    x[2, 5] = 1e-30                                        # far below the block maximum
    x[3, 7] = 3e20                                         # a huge element drags the block scale up
    x[4, :32] = 448.0 * 2 ** -3                            # the representable maximum
    x[5, :8] = torch.tensor([1.0625, 1.1875, 1.3125, 1.4375, 1.5625, 1.6875, 1.8125, 1.9375]) * 256      # ties of the 3-bit mantissa
    x[6, :32] = torch.linspace(0, 31, 32) * 2.0 ** -9 * 4  # the subnormal grid and its ties, block maximum 2^-2 ... : codes 0 ... 8 and the first normals
    x[7, :32] = 1.9921875 * 256                            # bf16 values above 448 X: saturate
    x[8, :32] = 1e-40                                      # a block of fp32 subnormals: scale byte 0
    return x


def test_mx8_statements_match_the_emulation_bit_for_bit():
    x = _mx8_inputs()
    q_ref, e_ref = E.mx8_quantize(x)
    q, e = F.mx8_quantize(x.double())
    assert torch.equal(q, q_ref.double()) and torch.equal(e, e_ref.double())
    assert 0.0 in q and 128.0 in q and 126.0 in q and 254.0 in q and any(float(v) in q for v in range(1, 8))        # zeros of both signs, saturation, subnormals
    assert torch.equal(F.mx8_dequantize(q, e), E.mx8_dequantize(q_ref, e_ref))
    # every code, through both dequantisers
    codes = torch.arange(256).repeat(1, 1).view(8, 32).to(torch.uint8)
    codes = codes[(codes & 0x7f) != 0x7f].view(-1)                    # (the two NaN codes are never stored: the quantiser saturates)
    codes = torch.cat([codes, codes[:2]]).view(-1, 32)
    sc = torch.full((codes.shape[0], 1), 127, dtype=torch.uint8)
    assert torch.equal(F.mx8_dequantize(codes.double(), sc.double()), E.mx8_dequantize(codes, sc))
    # the model of a producer is the emulation of its rounded output
    ref = torch.randn(16, 256, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    assert torch.equal(F.mx8_model(ref), E.mx8_dequantize(*E.mx8_quantize(ref.float().bfloat16().float())))
    rel = float(((F.mx8_model(ref) - ref) ** 2).sum().sqrt() / (ref ** 2).sum().sqrt())
    assert 1e-2 < rel < 2.0 ** -4, rel                               # three mantissa bits: half an ulp is at most 2^-4


def test_mx8_statements_match_the_library_host_quantiser():
    import ctypes as C
    from transformer_latent_diffusion_amd import _lib
    x = _mx8_inputs()
    R_, K = x.shape
    out, sc = np.zeros((R_, K), np.uint8), np.zeros((K // 128, R_, 4), np.uint8)
    xa = np.ascontiguousarray(x.numpy(), dtype=np.float32)
    _lib.check(_lib.lib().tld_debug_quant_mx8_host(xa.ctypes.data_as(C.POINTER(C.c_float)), R_, K, out.ctypes.data, sc.ctypes.data), "quant_mx8_host")
    q, e = F.mx8_quantize(x.double())
    assert np.array_equal(out, q.numpy().astype(np.uint8))
    assert np.array_equal(sc, E.scales_to_gemm_layout(e.to(torch.uint8)).numpy())


def test_mx8_linear_and_difference_report():
    gen = torch.Generator().manual_seed(10)
    a = F.bf16(torch.randn(48, 256, generator=gen, dtype=torch.float64))
    w = torch.randn(64, 256, generator=gen, dtype=torch.float64) * 0.05
    bias, resid = torch.randn(64, generator=gen, dtype=torch.float64), torch.randn(48, 64, generator=gen, dtype=torch.float64)
    q, s = F.mx8_quantize(a)
    wd = F.mx8_dequantize(*F.mx8_quantize(w))
    ref = R.linear_fwd(E.mx8_dequantize(q.to(torch.uint8), s.to(torch.uint8)), wd, bias) + resid
    assert torch.allclose(F.mx8_linear(q, s, wd, bias, resid), ref, rtol=0, atol=1e-13)
    rel = float(((F.mx8_linear(q, s, wd) - a @ w.T) ** 2).sum().sqrt() / ((a @ w.T) ** 2).sum().sqrt())
    assert rel < 6e-2, rel                                           # two e4m3 operands: a few percent by construction
    assert F.mx8_first_difference(q, s, q, s) == (0, 0, "")
    q2, s2 = q.clone(), s.clone()
    s2[5, 3] += 1; q2[7, 40] = 1.0 if q2[7, 40] != 1.0 else 2.0
    nq, ns, where = F.mx8_first_difference(q2, s2, q, s)
    assert (nq, ns) == (1, 1) and where.startswith("first at (row 5, block 3): scale"), where
    nq, ns, where = F.mx8_first_difference(q2, s, q, s)
    assert (nq, ns) == (1, 0) and where.startswith("first at (row 7, block 1): byte"), where
    assert F.dw_partial_tile_mask(32) is None
    m = F.dw_partial_tile_mask(24)
    assert m.shape == (24, 24) and int(m.sum()) == 24 * 24 - 16 * 16 and bool(m[23, 0]) and bool(m[0, 16]) and not bool(m[15, 15])

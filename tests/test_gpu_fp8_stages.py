"""GPU: the MX-fp8 forward stage by stage against float64, every producer of the quantised operand, every block, on the engine's own inputs.

The construction is that of tests/test_gpu_forward_stages.py (whose Checks, Body, conditioning / ends checks and tolerance constants are used as
they are: EXACT 2e-5 max|ref|, ROUND 2^-8 |ref| + 2e-5 sqrt(max(K, 64) / 64) max|ref|, MODELLED at twice the rounding model's own relative rms, whole
tensor and class by class; no constant is introduced here).  In fp8 mode tld_engine_set_debug also keeps, per block, the three A operands as the
GEMMs read them (blk<i>.a8_qkv / a8_up / a8_down: .q the e4m3 codes, .s the E8M0 bytes in logical [rows, K / 32] order), hid_pre, the bf16 stages
xn1 / xn3 / hid wherever a bf16 copy exists, and returns the e4m3 weights dequantised.  Every case runs twice on the same inputs, with
TLD_FP8_FUSED=0 (bf16 producers + launch_quant_mx8) and =1 (quantising producers), forwards inside the environment scope.  Per block:

* bf16 stages (xn1, xn3, hid where they exist; att, sa, ca): the classes of the bf16 file.
* quantisation: each a8_* of the unfused engine equals infer_stage_refs.mx8_quantize of the engine's own bf16 snapshot, bit for bit, every row
  (that function is held bit for bit against tests/mx8_emulation.py on the host; block 0's a8_qkv is also compared with mx8_emulation itself).
* producers: each a8_* of the fused engine equals the unfused engine's, bit for bit, codes and scales; the message gives the counts and the first
  differing (row, 32-block) and whether a code or a scale differs.
* producers against float64, independently of the other engine: the dequantised operand against the float64 LayerNorm / cross-row / depthwise + GELU
  result, MODELLED with the yardstick |mx8_dequantize(mx8_quantize(bf16(ref))) - ref|: whole tensor, first / last row, last partial 256-row tile,
  sample, cross_row workgroup boundary rows, the unconditional half, the zero-label samples, and for the depthwise operand corner / edge /
  interior / tile-seam pixels and the partial 16 x 16 tiles of the tiled kernel.
* fp8 GEMMs on the engine's operands: qk | vt, hid_pre and mlp against the float64 product of the dequantised a8_* snapshot and the dequantised
  weights as held (+ bias, + residual), ROUND with the layer's K.  The weights as held equal the quantiser's statement of the fp32 weights.
* stages that do not exist on a path (xn1 / xn3 where the producer quantises, hid where the depthwise kernel does) read as "no such stage".

Rows of a call that are not a multiple of 4 (tld_debug_gemm_mx8 and tld_debug_gemm_epilogue refuse them) cannot reach the engine's fp8 GEMMs:
tld_engine_create admits only token grids whose side is a multiple of 4 ("token count %d unsupported": ntok % 16 == 0), so batch x tokens is a
multiple of 16 for every batch, in the forward and in both halves of a sampler step.  test_odd_token_grids_are_refused holds that check.

The C4 sampler case (16 x 4096 = 65 536 rows) is the shape at which the fp8 down projection takes 256-wide tiles and the QKV / up projections the
ring K loop with the half-tile tail (tld_gemm_plan.h); the C1b case runs 37 samples on an engine of 128.

With TLD_FORWARD_STAGE_RECORD=<file> a summary per case is appended to that file, as in the bf16 file.  No run of this file on an MI355X is
recorded yet: the worst EXACT / ROUND ratios, the yardstick / measured pairs of the MODELLED transitions, the wall time and the record of the
in-bounds mutations (tiled scale byte from the neighbouring column, streaming scale offset, cross_row quantising the unrounded value, a LayerNorm
block maximum over 28 values, the scale layout indexed with the engine's capacity rows) are still to be measured and committed under profiles/.
"""
import gc

import numpy as np
import pytest
import torch

import infer_stage_refs as F
import mx8_emulation as E
import test_gpu_forward_stages as FS
import train_stage_refs as R
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

_cfg = FS._cfg
# name: (config, batch, max_batch, engines run: unfused and fused, or fused alone)
CASES = {
    "C1b": (_cfg(768, 32, 2), 37, 128, ("0", "1")),                      # grid 16: whole-image depthwise + separate pass on hid; quantising LN<3>, cross_row<3> writer; batch < max_batch
    "C3": (_cfg(768, 64, 2), 4, 8, ("0", "1")),                          # grid 32: streaming fp8 depthwise
    "C4": (_cfg(768, 128, 2), 8, 8, ("0", "1")),                         # grid 64, 4096 tokens, the C4 shape
    "T24": (_cfg(256, 48, 2), 3, 8, ("0", "1")),                         # grid 24: tiled fp8 depthwise, partial last tile; quantising LN<1>, cross_row<1> writer
    "T40": (_cfg(512, 80, 2, C=8), 2, 8, ("0", "1")),                    # grid 40, 8 channels; LN<2>, cross_row<2>
    "T48": (_cfg(256, 96, 2), 2, 8, ("0", "1")),                         # grid 48: full tiles
    "W384": (_cfg(384, 16, 2, patch=1, C=8, mult=2), 5, 8, ("0", "1")),  # fall-back width in a fused engine: generic LN + pass, VALU cross_row + pass; mlp_multiplier 2
    "W640": (_cfg(640, 48, 2, mult=2), 2, 8, ("0", "1")),                # ... with the tiled fp8 depthwise
    "W128": (_cfg(128, 64, 2), 2, 8, ("0", "1")),                        # ... with the streaming one
    "C4x12": (_cfg(768, 128, 12), 4, 8, ("1",)),                         # every block of the 100M model at 4096 tokens, the headline (fused) engine
}
SAMPLERS = {   # name: (config, B, levels, debug step)
    "T24s": (_cfg(256, 48, 2), 3, 4, 1),                                 # tiled; block 0's LayerNorm, QKV and attention on half the rows
    "C4s": (_cfg(768, 128, 2), 8, 4, 1),                                 # streaming; 65 536 rows
}
_PATHS = {}


class Checks8(FS.Checks):
    def same_operand(self, what, q, s, q_ref, s_ref):
        assert q.shape == q_ref.shape and s.shape == s_ref.shape, (what, q.shape, q_ref.shape, s.shape, s_ref.shape)
        nq, ns, where = F.mx8_first_difference(q, s, q_ref, s_ref)
        self.rows.append((what, "equal", float(nq + ns), 0.0))
        if nq + ns:
            self.fail.append(f"{self.name} {what} [bitwise]: {nq} of {q.numel()} codes and {ns} of {s.numel()} scale bytes differ; {where}")

    def classes(self, got, ref, samples, heads, pixels):
        out = super().classes(got, ref, samples, heads, pixels)
        m = F.dw_partial_tile_mask(self.G) if pixels else None
        if m is not None:
            m = m.reshape(-1).to(got.device)
            e3, r3 = ((got - ref) ** 2).view(samples, self.N, -1), (ref ** 2).view(samples, self.N, -1)
            out["partial 16 x 16 tiles"] = (e3[:, m].sum() / r3[:, m].sum().clamp_min(1e-300)).sqrt().reshape(1)
        return out


def _body(m, kw, tag, B, src, nrow, lrow, zero, checks=None):
    return FS.Body(m, kw, tag, B, src, nrow, lrow, zero, checks=checks or Checks8)


def check_block(b, i, fused, ops, ref_ops):
    """One block of an fp8 engine.  ops: this engine's operands are left there as uint8 for the other engine's comparison; ref_ops: the unfused engine's."""
    c, w, d, N, H, G, hid, B = b.c, b.w, b.d, b.N, b.H, b.G, b.hid, b.B
    p, s = f"{R.BLK}decoder_blocks.{i}.", f"blk{i}."
    S = lambda n: b.S(s + n)
    b0 = b.src if i == 0 else B
    M0, M = b0 * N, B * N
    ln8, cross8, dw8 = fused and d in (256, 512, 768), fused and d in (256, 512, 768), fused and G > 16
    for name, absent in (("xn1", ln8), ("xn3", cross8), ("hid", dw8)):
        assert b.has(s + name) == (not absent), f"{c.name} {s}{name}: captured {b.has(s + name)}, but the producer {'quantises' if absent else 'writes bf16'}"
    assert not b.has(s + "ln1") and not b.has(s + "stats") and b.has(s + "qk") and b.has(s + "hid_pre")

    def operand(name, rows, K, ref64, snap, samples, pixels=False):
        q, sc = S(name + ".q"), S(name + ".s")
        assert q.shape == (rows, K) and sc.shape == (rows, K // 32), (name, q.shape, sc.shape)
        ops[s + name] = (q.to(torch.uint8), sc.to(torch.uint8))
        if snap is not None:
            c.same_operand(s + name + " = mx8_quantize(bf16 snapshot)", q, sc, *F.mx8_quantize(snap))
        if ref_ops is not None:
            rq, rs = ref_ops[s + name]
            c.same_operand(s + name + ": quantising producer = separate pass", q, sc, rq.double(), rs.double())
        c.modelled(s + name + " against float64", F.mx8_dequantize(q, sc), ref64, F.mx8_model(ref64), samples, pixels=pixels)
        return q, sc

    def weight(name, key, rows, K):
        wd = S(name)
        c.equal(s + name + " = dequantised mx8_quantize(W)", wd, F.mx8_dequantize(*F.mx8_quantize(w[p + key].reshape(rows, K))))
        return wd

    x_in = S("x_in")
    c.equal(s + "x_in = previous stage", x_in, b.S("tokens0") if i == 0 else b.S(f"blk{i - 1}.mlp"))
    ln1 = R.ln_fwd(x_in, w[p + "norm1.weight"], w[p + "norm1.bias"])[0]
    xn1 = None if ln8 else S("xn1")
    if xn1 is not None:
        c.round(s + "xn1 = LN1(x)", xn1, ln1)
    q, sc = operand("a8_qkv", M0, d, ln1, xn1, b0)
    if i == 0 and xn1 is not None:       # the emulation itself, once per case (its float8 conversion runs on the host)
        eq, es = E.mx8_quantize(xn1.float().cpu())
        c.same_operand(s + "a8_qkv = mx8_emulation.mx8_quantize(xn1)", q.cpu(), sc.cpu(), eq.double(), es.double())
    qkv = F.mx8_linear(q, sc, weight("wqkv", "self_attention.qkv_linear.weight", 3 * d, d))
    qk, vt = S("qk"), S("vt")
    c.round(s + "fp8 QKV q | k", qk, qkv[:, :2 * d], K=d)
    v_eng = vt.permute(0, 2, 1).reshape(M0, d)
    c.round(s + "fp8 QKV V^T", v_eng, qkv[:, 2 * d:], K=d)
    exact, model = FS._attn_both(qk[:, :d].view(b0, N, d), qk[:, d:].view(b0, N, d), v_eng.view(b0, N, d), H, False)
    att = S("att")
    c.modelled(s + "self-attention", att, exact.reshape(M0, d), F.bf16(model).reshape(M0, d), b0, heads=True)
    del exact, model, qkv, qk, vt
    rep = B // b0
    x1, x2 = F.cross_row(x_in.view(b0, N, d).repeat(rep, 1, 1), att.view(b0, N, d).repeat(rep, 1, 1), b.wq[i], b.bwq[i], b.kv[i][:, d:], b.nrow, b.lrow)
    c.exact(s + "sa = x + att", S("sa"), x1.reshape(M, d))
    ca = S("ca")
    c.round(s + "ca = sa + cross-attention", ca, x2.reshape(M, d), K=d)
    ln3 = R.ln_fwd(x2.reshape(M, d), w[p + "norm3.weight"], w[p + "norm3.bias"])[0]      # (of the row the kernel holds, before the store rounds it)
    xn3 = None if cross8 else S("xn3")
    if xn3 is not None:
        c.round(s + "xn3 = LN3(sa + cross-attention)", xn3, ln3)
    q, sc = operand("a8_up", M, d, ln3, xn3, B)
    del x1, x2, ln1, ln3
    pre = S("hid_pre")
    c.round(s + "fp8 up projection", pre, F.mx8_linear(q, sc, weight("wup", "mlp.mlp.0.weight", hid, d), w[p + "mlp.mlp.0.bias"]), K=d)
    dww, dwb = w[p + "mlp.mlp.1.weight"].reshape(hid, 9), w[p + "mlp.mlp.1.bias"]
    exact = F.dw_gelu(pre.view(B, N, hid), dww, dwb, G).reshape(M, hid)
    hidt = None if dw8 else S("hid")
    if hidt is not None:
        if G <= 16:
            c.round(s + "depthwise + GELU (whole image)", hidt, exact)
        else:
            model = F.bf16(F.dw_gelu_model(pre.view(B, N, hid), dww, dwb, G, False)).reshape(M, hid)
            c.modelled(s + "depthwise + GELU (halved tables)", hidt, exact, model, B, pixels=True)
            del model
    del pre
    q, sc = operand("a8_down", M, hid, exact, hidt, B, pixels=True)
    del exact, hidt
    c.round(s + "fp8 mlp = ca + down projection", S("mlp"),
            F.mx8_linear(q, sc, weight("wdown", "mlp.mlp.3.weight", d, hid), w[p + "mlp.mlp.3.bias"], ca), K=hid)


def _engine(kw, max_batch, fused):
    m = FS._model(kw)
    m.set_gemm_dtype("fp8")
    m.reserve(max_batch)            # TLD_FP8_FUSED is read at tld_engine_create: the caller holds the environment scope over this and the forwards
    m.set_debug(True)
    return m


def _release(m):
    m.set_debug(False)
    del m
    gc.collect(); torch.cuda.empty_cache()


def run_forward_case(name, blocks=None, case=None, checks=None, paths=None):
    """case: a row like those of CASES, run under the tag `name` (tests/test_gpu_forward_grids.py); checks: a subclass of Checks8; paths: where the
    launch-path masks go (this file's record otherwise)."""
    kw, B, max_batch, engines = CASES[name] if case is None else case
    paths = _PATHS if paths is None else paths
    dev = _dev()
    x, sigma, lab, zero = FS._inputs(kw, B, 60 + B)
    xd, sd_, ld = x.to(dev), sigma.to(dev), lab.to(dev)
    ref_ops = None
    for fused in engines:
        def run():
            m = _engine(kw, max_batch, fused)
            try:
                out = m(xd, sd_, ld)
                torch.cuda.synchronize()
                b = _body(m, kw, f"{name}/{'fused' if fused == '1' else 'unfused'}", B, B, torch.arange(B), torch.arange(B) + B, zero, checks)
                paths[b.c.name] = b.paths
                FS.check_cond(b, sd_.reshape(-1), ld)
                FS.check_ends(b, xd, out)
                ops = {}
                for i in (range(b.L) if blocks is None else blocks):
                    check_block(b, i, fused == "1", ops, ref_ops)
                    torch.cuda.empty_cache()
                FS.report(b.c)
                return ops
            finally:
                _release(m)
        ref_ops = FS._with_env({"TLD_FP8_FUSED": fused}, run)


@pytest.mark.parametrize("name", list(CASES))
def test_fp8_forward_stages(name):
    run_forward_case(name)


def run_sampler_case(name, blocks=None):
    from transformer_latent_diffusion_amd import schedule
    kw, B, n_levels, step = SAMPLERS[name]
    dev = _dev()
    g = 3.0
    gen = torch.Generator().manual_seed(70 + B)
    S_, C = kw["image_size"], kw["n_channels"]
    xT = torch.randn(B, C, S_, S_, generator=gen).to(dev)
    lab = (torch.randn(B, 768, generator=gen) * 0.5).to(dev)
    co = schedule.step_coefficients(schedule.noise_schedule(n_levels, 1), True)
    n = co.shape[0]
    ref_ops = None
    for fused in ("0", "1"):
        def run():
            m = _engine(kw, 2 * B, fused)
            try:
                m.set_debug_step(step)
                lat, tx0, txt = m.sample_latents(xT, lab, co, g, trace=True)
                torch.cuda.synchronize()
                lrow = n + torch.cat([torch.arange(B), torch.full((B,), B)])
                b = _body(m, kw, f"{name}/{'fused' if fused == '1' else 'unfused'}/step{step}", 2 * B, B, torch.full((2 * B,), step), lrow, tuple(range(B, 2 * B)))
                _PATHS[b.c.name] = b.paths
                c = b.c
                FS.check_cond(b, torch.tensor([co[i][0] for i in range(n)], device=dev), torch.cat([lab, torch.zeros(1, 768, device=dev)]))
                x_t = b.S("step.x_t").view(B, C, S_, S_)
                c.equal("x_t entering the step = trace", x_t, txt[step - 1].double())
                FS.check_ends(b, x_t, None)
                ops = {}
                for i in (range(b.L) if blocks is None else blocks):
                    check_block(b, i, fused == "1", ops, ref_ops)
                    torch.cuda.empty_cache()
                out2 = b.S("step.out")
                c.equal("step.out = out stage", out2, b.S("out"))
                x0 = b.S("step.x0").view(B, C, S_, S_)
                c.exact("x0 = CFG combination", x0, F.cfg_combine(out2.view(2 * B, C, S_, S_), g))
                c.exact("x_next = update (second order)", b.S("step.x_next").view(B, C, S_, S_),
                        F.update_from(x_t, x0, b.S("step.x0_prev").view(B, C, S_, S_), co[step], float(co[step + 1][0]), None, None, None))
                FS.report(c)
                return ops
            finally:
                _release(m)
        ref_ops = FS._with_env({"TLD_FP8_FUSED": fused}, run)


@pytest.mark.parametrize("name", list(SAMPLERS))
def test_fp8_sampler_step(name):
    run_sampler_case(name)


def test_cases_reach_every_fp8_path():
    """The union of the cases' launch paths holds every writer of the fp8 operand, and the fused engines alone hold the four quantising producers."""
    from transformer_latent_diffusion_amd import Denoiser
    for name in CASES:
        if not any(k.startswith(name + "/") for k in _PATHS):
            run_forward_case(name, blocks=())
    for name in SAMPLERS:
        if not any(k.startswith(name + "/") for k in _PATHS):
            run_sampler_case(name, blocks=())
    names = Denoiser.FP8_PATH_NAMES
    assert sorted(names) == [10, 54, 55, 56, 57] and Denoiser.PATH_NAMES[10] == names[10] and len(Denoiser.PATH_NAMES) == 54
    union = fused = unfused = 0
    for k, v in sorted(_PATHS.items()):
        FS._record(f"launch paths {k:28s} {v:#018x}")
        union |= v
        if "/fused" in k:
            fused |= v
        else:
            unfused |= v
    producers = [i for i in names if i != 54]
    print(f"fp8 launch paths: union {union:#x}, fused engines {fused:#x}, unfused engines {unfused:#x}")
    assert not [names[i] for i in names if not union >> i & 1], "fp8 paths no case reaches"
    assert not [names[i] for i in producers if not fused >> i & 1], "quantising producers no fused case reaches"
    assert fused >> 54 & 1, "no fused case takes the separate pass (whole-image depthwise, fall-back widths)"
    assert not [names[i] for i in producers if unfused >> i & 1], "an unfused engine launched a quantising producer"
    for tag, bit in (("T24/fused", 56), ("T40/fused", 56), ("T48/fused", 56), ("W640/fused", 56), ("T24s/fused/step1", 56), ("C3/fused", 57), ("C4/fused", 57),
                     ("W128/fused", 57), ("C4s/fused/step1", 57), ("C1b/fused", 54), ("W384/fused", 54), ("C1b/fused", 55), ("T24/fused", 10), ("T40/fused", 10)):
        assert _PATHS[tag] >> bit & 1, (tag, names[bit])
    for tag in ("W384/fused", "W640/fused", "W128/fused"):      # the fall-back widths: no quantising LayerNorm, no cross_row writer
        assert not _PATHS[tag] >> 10 & 1 and not _PATHS[tag] >> 55 & 1, tag
    for tag in ("T24s/fused/step1", "C4s/fused/step1"):         # layer-0 sharing was on
        assert _PATHS[tag] >> 27 & 1, tag


def test_odd_token_grids_are_refused():
    """batch x tokens % 4 != 0 cannot reach the fp8 GEMMs: an odd token grid (patch 1 on an odd image side) is refused when the engine is created."""
    from transformer_latent_diffusion_amd import Denoiser
    for image, patch in ((15, 1), (30, 2), (18, 1)):
        m = Denoiser(**_cfg(128, image, 1, patch=patch)).to(_dev()).set_gemm_dtype("fp8")
        with pytest.raises(RuntimeError, match="multiple of 4"):
            m.reserve(1)


def test_fp8_stage_names():
    """Shapes of the fp8 stages, the row count of a call below max_batch, and "no such stage" for what a path does not write."""
    kw = _cfg(256, 48, 1)
    x, sigma, lab, _ = FS._inputs(kw, 3, 5)
    dev = _dev()

    def run():
        m = _engine(kw, 8, "1")
        try:
            m(x.to(dev), sigma.to(dev), lab.to(dev))
            N = 24 * 24
            assert m.stage_shape("blk0.a8_qkv.q") == (3 * N, 256) and m.stage_shape("blk0.a8_qkv.s") == (3 * N, 8)
            assert m.stage_shape("blk0.a8_down.q") == (3 * N, 1024) and m.stage_shape("blk0.a8_down.s") == (3 * N, 32)
            assert m.stage_shape("blk0.hid_pre") == (3 * N, 1024) and m.stage_shape("blk0.wdown") == (256, 1024)
            q = m.read_stage("blk0.a8_up.q")
            assert q.min() >= 0 and q.max() <= 255 and np.array_equal(q, np.round(q))
            for absent in ("blk0.xn1", "blk0.xn3", "blk0.hid", "blk0.ln1", "blk0.stats", "blk1.a8_qkv.q"):
                with pytest.raises(RuntimeError, match="status 2"):
                    m.read_stage(absent)
            with pytest.raises(RuntimeError, match="status 3"):
                m.read_stage("blk0.a8_up.s", (3 * N, 2))
        finally:
            _release(m)
    FS._with_env({"TLD_FP8_FUSED": "1"}, run)

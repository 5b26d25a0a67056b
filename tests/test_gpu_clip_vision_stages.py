"""GPU: the CLIP image tower (csrc/tld_clip_vision.hip) stage by stage against float64, on the engine's own inputs.

Every transition of every block starts from the engine's snapshot of its inputs (tld_clip_vis_set_debug; stage names in include/tld_hip.h) and the
operands as the engine holds them, is recomputed in float64 on the device with tests/clip_vision_refs.py / tests/clip_stage_refs.py (held against
transformers in tests/test_clip_vision_host.py) and compared with the engine's snapshot of its output, so errors do not pile up along the chain.
Every tensor is first checked for NaN / Inf: the hook fills the workspace of all max_batch samples with 0xFF bytes and every case runs fewer
samples than max_batch, so a read past a sample's rows or past the batch lands in NaN instead of leaving the allocation.

Tolerance classes and constants are those of tests/test_gpu_clip_stages.py (no new numbers): EXACT x0, x1, x2, pooled, out; ROUND patches, h1, h2,
qkv, f_pre, f with the K of the producing GEMM; GEMM32 emb, attn_out, mlp_out.  Attention is MODELLED as in tests/test_gpu_forward_stages.py: the
bound is MODEL_FACTOR (2) x the relative rms between ``attention_model`` (the kernel's documented roundings) and ``attention_exact``, over the whole
tensor and member by member -- each (sample, head), each sample's class-token row, last row and rows of the last partial 32-query tile; where the
model's own error over the whole tensor is below 2^-11 the ROUND bound holds instead.

test_attention_kernel runs clip_vis_attn_kernel alone (tld_debug_clip_vis_attention) at the cases' token counts, the tile edges around them
(32, 33, 64, 256) and n = 2, with one and two heads, on random inputs and on the three adversarial ones of tests/test_clip_vision_host.py
(attention_inputs): the last key dominates every row (a kernel that drops or mis-masks the last partial tile fails), key 0 dominates, and every
real score is about -98 (a row maximum taken over padded keys fails).  The qkv buffer there carries one more, NaN-filled, sample behind the batch
and the output buffer NaN-bit rows behind the batch that must keep their bits.

Cases (tests/test_clip_vision_host.py CASES): token counts 5, 17, 50, 65 at width 64 and 128, 197 and 257 at width 128, width 1024 at 257 tokens,
24 layers at width 256 and 257 tokens; contraction lengths 588 (padded to 640), 3072 and 768 in the patch GEMM.
"""
import ctypes as C
import os

import pytest
import torch

import clip_stage_refs as R
import clip_vision_refs as V
from test_clip_vision_host import ATTN_KINDS, ATTN_TOKENS, CASES, attention_inputs, case_pixels, case_weights
from test_gpu_clip_stages import ACC_TOL, EXACT_TOL, GEMM32_ABS, ROUND_REL
from test_gpu_forward_stages import MODEL_FACTOR
from test_gpu_parity import _dev
from transformer_latent_diffusion_amd import _lib
from transformer_latent_diffusion_amd.clip_image import ClipImageEncoder

gpu = pytest.mark.gpu


def _record(line):
    path = os.environ.get("TLD_CLIP_VISION_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _rms(t, dims):
    return t.double().pow(2).mean(dim=dims).sqrt()


def attention_classes(x, exact, batch, n, heads):
    """Relative rms of x - exact per member of every class: {class: tensor of one value per member}."""
    err, ref = (x.double() - exact).view(batch, n, heads, 64), exact.view(batch, n, heads, 64)
    t0 = 32 * ((n - 1) // 32)                                   # first row of the last (partial) 32-query tile
    rel = lambda sl, dims: _rms(err[sl], dims) / _rms(ref[sl], dims)
    return {"whole": rel((slice(None),), (0, 1, 2, 3)).reshape(1), "(sample, head)": rel((slice(None),), (1, 3)).reshape(-1),
            "class-token row": rel((slice(None), slice(0, 1)), (1, 2, 3)), "last row": rel((slice(None), slice(n - 1, n)), (1, 2, 3)),
            "last query tile": rel((slice(None), slice(t0, n)), (1, 2, 3))}


class Checks:
    def __init__(self, name):
        self.name, self.fail, self.rows = name, [], []

    def _finite(self, stage, got):
        bad = int((~torch.isfinite(got)).sum())
        if bad:
            self.fail.append(f"{self.name} {stage}: {bad} of {got.numel()} values are NaN / Inf")
        return not bad

    def compare(self, stage, tol, got, ref, bound):
        if not self._finite(stage, got):
            return
        assert got.shape == ref.shape, (stage, got.shape, ref.shape)
        v = float(((got.double() - ref).abs() / bound).max())
        self.rows.append((stage, tol, v))
        print(f"{self.name:9s} {stage:14s} {tol:8s} value / bound {v:.3f}")
        if not v <= 1.0:
            self.fail.append(f"{self.name} {stage} [{tol}]: value / bound = {v:.3g}")

    def exact(self, stage, got, ref):
        self.compare(stage, "EXACT", got, ref, torch.full_like(ref, EXACT_TOL * float(ref.abs().max())))

    def round(self, stage, got, ref, K):
        self.compare(stage, "ROUND", got, ref, ROUND_REL * ref.abs() + ACC_TOL * (max(K, 64) / 64) ** 0.5 * float(ref.abs().max()))

    def gemm32(self, stage, got, ref, K):
        self.compare(stage, "GEMM32", got, ref, torch.full_like(ref, ACC_TOL * float(ref.abs().max()) * (K / 64) ** 0.5 + GEMM32_ABS))

    def modelled(self, stage, got, exact, model, batch, n, heads):
        if not self._finite(stage, got):
            return
        yard = attention_classes(model, exact, batch, n, heads)
        if float(yard["whole"]) < 2.0 ** -11:                   # the model says nothing (tests/test_gpu_forward_stages.py): ROUND then
            return self.round(stage + " (model error near zero)", got, exact, n)
        meas = attention_classes(got, exact, batch, n, heads)
        for cls in yard:
            ratio = meas[cls] / (MODEL_FACTOR * yard[cls])
            i = int(ratio.argmax())
            v = float(ratio[i])
            self.rows.append((stage, "MODELLED", v))
            print(f"{self.name:9s} {stage:14s} MODELLED {cls:16s} measured {float(meas[cls][i]):.3e} yardstick {float(yard[cls][i]):.3e} (member {i})")
            if not v <= 1.0:
                self.fail.append(f"{self.name} {stage} [MODELLED] {cls} member {i}: measured {float(meas[cls][i]):.3e} > {MODEL_FACTOR} x {float(yard[cls][i]):.3e}")

    def summary(self):
        worst = {}
        for stage, tol, v in self.rows:
            if tol not in worst or not v <= worst[tol][0]:
                worst[tol] = (v, stage)
        return [f"  {tol:8s} worst value / bound {v:.3f}  ({stage})" for tol, (v, stage) in sorted(worst.items())]


# ---- the attention kernel alone ------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_kernel(kind, heads):
    dev, L, batch = _dev(), _lib.lib(), 3
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    fails = []
    for n in ATTN_TOKENS:
        qkv = attention_inputs(n, heads, kind, batch)
        W, T = heads * 64, batch * n
        buf = torch.full(((batch + 1) * n, 3 * W), float("nan"), dtype=torch.bfloat16, device=dev)      # one NaN sample behind the batch
        buf[:T] = qkv.to(dev).to(torch.bfloat16)
        out = torch.full(((batch + 1) * n, W), -1, dtype=torch.int16, device=dev)                         # 0xFFFF: a NaN in bf16
        _lib.check(L.tld_debug_clip_vis_attention(C.c_void_p(buf.data_ptr()), C.c_void_p(out.data_ptr()), batch, n, heads, stream), "attention")
        torch.cuda.synchronize()
        assert bool((out[T:] == -1).all()), f"n {n}: rows behind the batch were stored"
        got = out[:T].view(torch.bfloat16).float()
        q64 = qkv.to(dev)
        c = Checks(f"{kind}/{heads}h/n{n}")
        c.modelled("att", got, V.attention_exact(q64, batch, n), V.attention_model(q64, batch, n), batch, n, heads)
        fails += c.fail
        _record(f"attention {kind} heads {heads} n {n}: " + "; ".join(s.strip() for s in c.summary()))
    assert not fails, "\n".join(fails[:40])


# ---- the engine, stage by stage ------------------------------------------------------------------------------------------------------

def make_encoder(name):
    cfg, _, max_batch, _ = CASES[name]
    w = case_weights(name)
    return w, ClipImageEncoder(cfg, max_batch=max_batch).load_state_dict(w).to(_dev())


def check_encode(name, cfg, w, enc, pixels, out):
    dev = _dev()
    B, n, W, L, p = pixels.shape[0], cfg.tokens, cfg.width, cfg.layers, cfg.patch_size
    Kp = V.padded_k(p)
    c = Checks(name)
    st = lambda s: enc.read_stage(s).to(dev)
    v = lambda k: w["visual." + k].to(dev)                     # fp32 operands: uploaded unchanged
    blk = lambda i, k: v(f"transformer.resblocks.{i}.{k}")

    pat = st("patches")
    assert pat.shape == (B * cfg.grid ** 2, Kp)
    c.round("patches", pat, V.patches(pixels.to(dev), p), 64)
    conv_w = st("conv_w")
    assert torch.equal(conv_w, V.bf16(V.pack_conv_weight(v("conv1.weight"), p)).float()), "conv_w is not conv1.weight rounded to bf16 and zero-padded"
    emb = st("emb")
    c.gemm32("emb", emb, V.patch_embed(pat, conv_w), Kp)
    x = st("x0")
    assert x.shape == (B * n, W)
    c.exact("x0", x, V.embed_ln_pre(emb, v("class_embedding"), v("positional_embedding"), v("ln_pre.weight"), v("ln_pre.bias"), B))
    h = st("blk0.h1")
    c.round("blk0.h1", h, R.layer_norm(x, blk(0, "ln_1.weight"), blk(0, "ln_1.bias")), W)
    for i in range(L):
        s = f"blk{i}."
        qkv = st(s + "qkv")
        c.round(s + "qkv", qkv, R.in_proj(h, st(s + "in_w"), blk(i, "attn.in_proj_bias")), W)
        att = st(s + "att")
        c.modelled(s + "att", att, V.attention_exact(qkv, B, n), V.attention_model(qkv, B, n), B, n, cfg.heads)
        ao = st(s + "attn_out")
        c.gemm32(s + "attn_out", ao, R.out_proj(att, st(s + "out_w")), W)
        x1, h2 = st(s + "x1"), st(s + "h2")
        c.exact(s + "x1", x1, R.add_layer_norm(x, ao, blk(i, "attn.out_proj.bias"), blk(i, "ln_2.weight"), blk(i, "ln_2.bias"))[0])
        c.round(s + "h2", h2, R.layer_norm(x1, blk(i, "ln_2.weight"), blk(i, "ln_2.bias")), W)
        f_pre = st(s + "f_pre")
        c.round(s + "f_pre", f_pre, R.c_fc(h2, st(s + "fc_w"), blk(i, "mlp.c_fc.bias")), W)
        f = st(s + "f")
        c.round(s + "f", f, R.quick_gelu(f_pre), 64)
        mo = st(s + "mlp_out")
        c.gemm32(s + "mlp_out", mo, R.c_proj(f, st(s + "proj_w")), 4 * W)
        del qkv, att, ao, h2, f_pre, f
        if i + 1 < L:
            x, h = st(s + "x2"), st(f"blk{i + 1}.h1")
            c.exact(s + "x2", x, x1.double() + mo.double() + blk(i, "mlp.c_proj.bias").double())
            c.round(f"blk{i + 1}.h1", h, R.layer_norm(x, blk(i + 1, "ln_1.weight"), blk(i + 1, "ln_1.bias")), W)
        else:
            pooled = st("pooled")
            c.exact("pooled", pooled, V.class_add_layer_norm(x1, mo, blk(i, "mlp.c_proj.bias"), v("ln_post.weight"), v("ln_post.bias"), n))
            got = st("out")
            c.exact("out", got, R.projection(pooled, st("proj_t")))
            assert torch.equal(got, out), "the 'out' stage is not what encode_image returned"
    return c


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_of_every_block(name):
    cfg, batch, max_batch, _ = CASES[name]
    assert batch < max_batch
    w, enc = make_encoder(name)
    enc.set_debug(True)
    pixels = case_pixels(name)
    out = enc.encode_image(pixels.to(_dev()))
    torch.cuda.synchronize()
    c = check_encode(name, cfg, w, enc, pixels, out)
    enc.set_debug(False)
    enc._drop_engine()
    lines = [f"{name}: tokens {cfg.tokens} width {cfg.width} layers {cfg.layers} batch {batch} of {max_batch}, {len(c.rows)} bounded values, "
             f"{len(c.fail)} above their bound"] + c.summary()
    print("\n".join(lines))
    for ln in lines:
        _record(ln)
    assert not c.fail, "\n".join(c.fail[:40])

"""GPU: the CLIP image tower end to end, its bitwise properties and its public surface.

End to end (test_encode_image_against_float64): ``encode_image`` of the depth (24 layers, width 256) and width (1024, 16 heads) cases at 257 tokens
against the float64 chain of tests/clip_vision_refs.py (held against transformers in tests/test_clip_vision_host.py).  The bound is not a constant:
it is twice the relative rms that the same float64 chain gives with the engine's roundings applied -- bf16 GEMM operands at the ROUND stages and
``attention_model`` at the attention (``chain(..., rounded=True)``).  Measured on an MI355X (relative rms, engine / rounding model):
DEPTH 7.81e-3 / 8.11e-3, WIDTH 8.09e-3 / 7.99e-3 -- the engine's error is the rounding model's.
With TLD_CLIP_VISION_RECORD=<file> the pair is appended to that file (profiles/clip_vision_stage_errors.txt is such a run).

Bitwise: two calls, debug on / off, a batch chunked over max_batch against its chunks alone, fp16 / bf16 pixels against fp32 pixels of the same values.
Surface: ``Clip`` as the pipeline's ``clip_model``, ``DiffusionTransformer.clip_scores``, ``Trainer.eval_clip_score``.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_vision_refs as V
from test_clip_vision_host import CASES, case_pixels, vcfg
from test_gpu_clip_vision_stages import _record, make_encoder
from test_gpu_parity import _dev
from transformer_latent_diffusion_amd import _lib
from transformer_latent_diffusion_amd.clip_image import Clip, ClipImageEncoder, clip_preprocess, clip_score

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.mark.parametrize("name", ["DEPTH", "WIDTH"])
def test_encode_image_against_float64(name):
    cfg, batch, _, _ = CASES[name]
    w, enc = make_encoder(name)
    pix = case_pixels(name)
    got = enc.encode_image(pix.to(_dev()))
    enc._drop_engine()
    assert bool(torch.isfinite(got).all())
    wd = {k: t.to(_dev()) for k, t in w.items()}
    exact = V.chain(cfg, wd, pix.to(_dev()))
    yard = _rel(V.chain(cfg, wd, pix.to(_dev()), rounded=True), exact)
    meas = _rel(got, exact)
    line = f"{name} end to end: encode_image against float64 rel-rms {meas:.3e}, rounding model {yard:.3e} (bound: twice the model)"
    print(line)
    _record(line)
    assert 0 < yard and meas <= 2 * yard, line


def test_bitwise_properties():
    name = "T50W128"
    cfg, _, max_batch, _ = CASES[name]
    w, enc = make_encoder(name)
    dev = _dev()
    pix = case_pixels(name, batch=3).to(dev)
    a = enc.encode_image(pix).clone()
    assert torch.equal(a, enc.encode_image(pix))                                        # two calls
    enc.set_debug(True)
    on = enc.encode_image(pix).clone()
    assert torch.equal(enc.read_stage("out").to(dev), on)
    enc.set_debug(False)
    with pytest.raises(RuntimeError, match="no captured stage"):
        enc.read_stage("x0")                                                           # debug off: nothing is kept
    assert torch.equal(a, on) and torch.equal(a, enc.encode_image(pix))                 # debug on / off
    big = case_pixels(name, batch=2 * max_batch + 1, seed=5).to(dev)                    # chunked in Python: 4 + 4 + 1
    whole = enc.encode_image(big)
    parts = torch.cat([enc.encode_image(big[i:i + max_batch]) for i in range(0, big.shape[0], max_batch)])
    assert whole.shape == (2 * max_batch + 1, cfg.embed_dim) and torch.equal(whole, parts)
    for dt in (torch.float16, torch.bfloat16):                                          # half-precision pixels = fp32 pixels holding the same values
        low = pix.to(dt)
        assert torch.equal(enc.encode_image(low), enc.encode_image(low.float())), dt
    assert not torch.equal(enc.encode_image(pix.to(torch.float16) * 1.5), a)                    # (other pixels do give other embeddings)
    assert enc.weight_bytes > 0
    enc._drop_engine()


def test_random_weights_warn_once():
    enc = ClipImageEncoder(vcfg(14, 2, 64), max_batch=2).to(_dev())
    x = torch.zeros(1, 3, 28, 28, device=_dev())
    with pytest.warns(RuntimeWarning, match="RANDOM initialisation"):
        enc.encode_image(x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        enc.encode_image(x)
    enc._drop_engine()


def test_abi_state_errors():
    L = _lib.lib()
    h = C.c_void_p()
    cc = _lib.TldClipVisConfig(28, 14, 64, 1, 1, 32, 2, _dev().index or 0)
    assert L.tld_clip_vis_create(C.byref(cc), C.byref(h)) == 0
    pix = torch.zeros(1, 3, 28, 28, device=_dev())
    out = torch.zeros(1, 32, device=_dev())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.tld_clip_vis_encode_image(h, pix.data_ptr(), out.data_ptr(), 1, 0, st) == 4 and b"not finalized" in L.tld_last_error()
    assert L.tld_clip_vis_finalize_weights(h) == 4 and b"missing state_dict entry" in L.tld_last_error()
    a = np.zeros((3, 3), np.float32)
    shp = (C.c_int64 * 2)(3, 3)
    ptr = a.ctypes.data_as(C.c_void_p)
    assert L.tld_clip_vis_load_tensor(h, b"nonsense", ptr, shp, 2, 0) == 2
    assert L.tld_clip_vis_load_tensor(h, b"visual.nonsense", ptr, shp, 2, 0) == 2
    assert L.tld_clip_vis_load_tensor(h, b"text_projection", ptr, shp, 2, 0) == 0                  # the text side: ignored
    assert L.tld_clip_vis_load_tensor(h, b"transformer.resblocks.0.ln_1.weight", ptr, shp, 2, 0) == 0
    assert L.tld_clip_vis_load_tensor(h, b"visual.class_embedding", ptr, shp, 2, 0) == 0
    assert L.tld_clip_vis_finalize_weights(h) == 3 and b"visual.class_embedding" in L.tld_last_error()
    assert L.tld_clip_vis_destroy(h) == 0


# ---- surface -------------------------------------------------------------------------------------------------------------------------

def _tiny_clip(max_batch=4):
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    tcfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    icfg = vcfg(14, 2, 128, embed_dim=768)
    text = ClipTextEncoder(tcfg, init_seed=1, max_batch=max_batch)
    text.load_state_dict(text.state_dict())                                             # (loaded weights: no warning)
    visual = ClipImageEncoder(icfg, init_seed=2, max_batch=max_batch)
    visual.load_state_dict(visual.state_dict())
    return tcfg, Clip(text, visual).to(_dev())


def test_clip_as_the_pipelines_clip_model():
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, DenoiserConfig, DiffusionTransformer, LTDConfig, VaeDecoderConfig
    tcfg, clip = _tiny_clip()

    class Tok:
        def tokenize(self, prompts, truncate=True):
            t = torch.zeros(len(prompts), tcfg.context_length, dtype=torch.long)
            for i, p in enumerate(prompts):
                ids = [1 + (ord(ch) % 900) for ch in p][: tcfg.context_length - 2]
                t[i, 0] = tcfg.vocab_size - 2
                t[i, 1:1 + len(ids)] = torch.tensor(ids)
                t[i, 1 + len(ids)] = tcfg.vocab_size - 1
            return t

    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2).to(_dev())
    cfg = LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4))
    pipe = DiffusionTransformer(cfg, vae=vae, clip_model=clip, tokenizer=Tok(), run_device=_dev())
    alone = DiffusionTransformer(cfg, vae=vae, clip_model=clip.text, tokenizer=Tok(), run_device=_dev())
    prompts = ["a cute cat", "a red car"]
    labels = pipe.encode_text(prompts)
    assert torch.equal(labels, alone.encode_text(prompts))                              # the text path is the text tower's
    images = torch.rand(2, 3, 40, 56, generator=torch.Generator().manual_seed(0))
    scores = pipe.clip_scores(images, prompts)
    want = clip_score(clip.encode_image(clip_preprocess(images.to(_dev()), 28)), labels.to(_dev()))
    assert scores.shape == (2,) and scores.device.type == "cuda" and torch.equal(scores, want)
    assert bool(torch.isfinite(scores).all()) and bool((scores.abs() <= 1 + 1e-6).all())
    with pytest.raises(RuntimeError, match="needs a clip_model with encode_image"):
        alone.clip_scores(images, prompts)
    with pytest.raises(ValueError, match="2 images but 1 prompts"):
        pipe.clip_scores(images, prompts[:1])


def test_trainer_eval_clip_score():
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, DenoiserConfig, TrainConfig, Trainer, VaeDecoderConfig
    dcfg = DenoiserConfig(image_size=16, noise_embed_dims=256, patch_size=2, embed_dim=256, dropout=0, n_layers=2, text_emb_size=768, n_channels=4)
    _, clip = _tiny_clip(max_batch=3)                                                   # 8 images: chunked 3 + 3 + 2
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2, max_batch=8).to(_dev())
    tr = Trainer(dcfg, TrainConfig(batch_size=8, lr=1e-3, alpha=0.9), device=_dev(), init_seed=4, max_batch=8)
    g = torch.Generator().manual_seed(3)
    batch = lambda: (torch.randn(8, 4, 16, 16, generator=g) * 0.5, torch.rand(8, generator=g) * 0.9 + 0.05, torch.randn(8, 768, generator=g) * 0.5)
    mk = lambda x, nl, y: (x + nl.view(-1, 1, 1, 1) * torch.randn(x.shape, generator=g), nl, y, x)
    tr.forward_backward(*mk(*batch())); tr.optimizer_step()
    tr.forward_backward(*mk(*batch()), last_micro_batch=False)                          # an accumulation in progress
    state = (tr.params.clone(), tr.ema.clone(), tr.step, tr.global_step, tr._acc_n, None if tr._acc is None else tr._acc.clone())
    labels = torch.randn(4, 768, generator=g) * 0.5
    lat, images, scores = tr.eval_clip_score(labels, vae, clip, num_imgs=8, n_iter=4)
    lat2, images2 = tr.eval_generate(labels, vae, num_imgs=8, n_iter=4)
    assert torch.equal(lat, lat2) and torch.equal(images, images2) and images.shape == (8, 3, 32, 32)
    pix = clip_preprocess((images.to(_dev()).float() * 0.5 + 0.5).clamp(0, 1), 28)
    want = clip_score(clip.visual.encode_image(pix), torch.repeat_interleave(labels, 2, dim=0).to(_dev()))
    assert scores.shape == (8,) and scores.device.type == "cuda" and scores.dtype == torch.float32 and torch.equal(scores, want)
    assert bool(torch.isfinite(scores).all())
    only = tr.eval_clip_score(labels, vae, clip.visual, num_imgs=8, n_iter=4)[2]         # the image tower alone is accepted too
    assert torch.equal(only, scores)
    assert torch.equal(tr.params, state[0]) and torch.equal(tr.ema, state[1]) and (tr.step, tr.global_step, tr._acc_n) == state[2:5]
    assert state[5] is None or torch.equal(tr._acc, state[5])
    with pytest.raises(ValueError, match="needs a vae"):
        tr.eval_clip_score(labels, None, clip)

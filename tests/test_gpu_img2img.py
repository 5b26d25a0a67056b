"""GPU: image-to-image and inpainting in the on-device sampler (tld_sample_from).

Bitwise anchors tie the new entry point to the existing one (strength 1.0 is ``generate_latents``; an all-ones mask is no mask; samples
do not interact; calls repeat), the known region is held exactly, and the trajectory is held to the project's contract tolerance
(TRAJ_TOL = 6e-2, tests/test_gpu_parity.py) against the reference's sampler loop extended on the CPU
(tests/img2img_ref.py).  Measured errors (MI355X) are recorded in DESIGN.md section 7.5; every test prints the figures it asserts."""
import warnings
from dataclasses import asdict

import numpy as np
import pytest
import torch

import img2img_ref as R
from conftest import cfg_from_arr, load_golden, synth_weights

pytestmark = pytest.mark.gpu

TRAJ_TOL = 6e-2          # the contract tolerance of a multi-step CFG trajectory (tests/test_gpu_parity.py)

_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(fixture, low_latency=0):
    """(cfg, state dict, Denoiser, DiffusionGenerator) for a golden fixture's configuration and synthetic weights."""
    key = (fixture, low_latency)
    if key not in _CACHE:
        from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
        g = load_golden(fixture)
        cfg = cfg_from_arr(g["cfg"])
        sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
        m = Denoiser(**asdict(cfg)).to(_dev())
        if low_latency:
            m.set_low_latency(low_latency)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        _CACHE[key] = (cfg, sd, m, DiffusionGenerator(m, None, _dev(), torch.float32))
    return _CACHE[key]


TINY, BIG = "g2_tiny32_sampler.npz", "g5_100m.npz"


def _inputs(B, S=32, seed=31):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S, S, generator=gen)
    z0 = torch.randn(B, 4, S, S, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


def _rect_masks(B, S=32):
    """0/1 rectangles, a different one per sample (1 = regenerate)."""
    m = torch.zeros(B, 1, S, S)
    for b in range(B):
        y0, x0 = (3 + 5 * b) % (S // 2), (7 * b) % (S // 2)
        m[b, :, y0:y0 + S // 2 - b, x0:x0 + S // 3 + 2 * b] = 1
    return m


def _frac_mask(B, S=32):
    """a soft-edged mask: 1 in the middle, 0 at the border rows / columns, a ramp between."""
    ramp = torch.clamp((torch.arange(S, dtype=torch.float32) - 4) / 8, 0, 1)
    ramp = torch.minimum(ramp, ramp.flip(0))
    return (ramp[:, None] * ramp[None, :]).expand(B, 1, S, S).contiguous()


def _rel_rms(a, b, sel):
    a, b = a.double()[sel], b.double()[sel]
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


# ---- bitwise anchors ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_full_strength_without_mask_is_generate_latents(plus):
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(2)
    kw = dict(n_iter=8, num_imgs=2, class_guidance=3.0, img_size=32, sharp_f=0.1, bright_f=0.1, seeds=eps, use_ddpm_plus=plus, trace=True)
    want = gen.generate_latents(labels, **kw)
    got = gen.generate_latents_from(z0, labels, strength=1.0, **kw)
    for a, b, what in zip(got, want, ("end latent", "trace_x0", "trace_xt")):
        assert a.shape == b.shape and torch.equal(a, b), f"{what} differs from generate_latents"
    # ... and with the generator's own noise (seed=), the same noise as text-to-image
    assert torch.equal(gen.generate_latents_from(z0, labels, strength=1.0, n_iter=5, seed=10, use_ddpm_plus=plus),
                       gen.generate_latents(labels, n_iter=5, num_imgs=2, seed=10, img_size=32, use_ddpm_plus=plus))


def test_all_ones_mask_is_no_mask():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(2)
    kw = dict(strength=0.65, n_iter=8, class_guidance=3.0, seeds=eps, sharp_f=0.1, bright_f=0.1, trace=True)
    a = gen.generate_latents_from(z0, labels, **kw)
    b = gen.generate_latents_from(z0, labels, mask=torch.ones(2, 1, 32, 32), **kw)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert not torch.equal(a[0], gen.generate_latents_from(z0, labels, **dict(kw, strength=1.0))[0])      # the start really moved


def test_samples_do_not_interact_and_calls_repeat():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    mask = _rect_masks(5)
    mask[3] = _frac_mask(1)[0]
    kw = dict(strength=0.65, n_iter=8, class_guidance=3.0, sharp_f=0.1, bright_f=0.1)
    full = gen.generate_latents_from(z0, labels, mask=mask, seeds=eps, **kw)
    assert torch.isfinite(full).all()
    assert torch.equal(full, gen.generate_latents_from(z0, labels, mask=mask, seeds=eps, **kw)), "two identical calls differ"
    for i in range(5):
        alone = gen.generate_latents_from(z0[i:i + 1], labels[i:i + 1], mask=mask[i:i + 1], seeds=eps[i:i + 1], **kw)
        assert torch.equal(alone[0], full[i]), f"sample {i} depends on its batch"


def test_low_latency_class_2_full_strength_is_its_generate_latents():
    cfg, sd, m, gen = _model(BIG, low_latency=2)
    eps, z0, labels = _inputs(1, seed=33)
    kw = dict(n_iter=4, num_imgs=1, class_guidance=6.0, img_size=32, sharp_f=0.0, bright_f=0.0, seeds=eps)
    want = gen.generate_latents(labels, **kw)
    assert torch.equal(gen.generate_latents_from(z0, labels, strength=1.0, **kw), want)
    out = gen.generate_latents_from(z0, labels, strength=0.6, mask=_rect_masks(1), **kw)                  # the class serves the masked path too
    assert torch.isfinite(out).all() and not torch.equal(out, want)


@pytest.mark.parametrize("entry", ["plain", "from"])
def test_long_schedule_has_no_conditioning_row_cap(entry):
    """1030 levels at batch 2 are 1030 + 2 + 1 > 1024 conditioning rows: the cap of tld_sample_requests (schedule.REQUEST_ROW_CAP) is that
    entry's alone.  tld_sample and tld_sample_from take the call, return something finite, and repeat it bit for bit."""
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(2, seed=35)
    n = 1030
    assert n + 2 + 1 > schedule.REQUEST_ROW_CAP
    kw = dict(n_iter=n, class_guidance=3.0, seeds=eps, sharp_f=0.1, bright_f=0.1)
    if entry == "plain":
        run = lambda: gen.generate_latents(labels, num_imgs=2, img_size=32, **kw)
    else:
        run = lambda: gen.generate_latents_from(z0, labels, strength=1.0, mask=_rect_masks(2), **kw)
    a = run()
    assert a.shape == eps.shape and torch.isfinite(a).all()
    assert torch.equal(a, run()), "two identical calls differ"


@pytest.mark.parametrize("entry", ["plain", "from", "from_mask"])
def test_scalar_instantiation_through_an_odd_offset_view(entry):
    """As in tests/test_gpu_requests.py: from Python only the 16-byte instantiation of the step kernel can be reached, so the scalar one is
    reached by handing the C entry an out_latent and a trace_x0 that start 4 bytes into their buffers: same bits as the aligned call."""
    import ctypes as C
    from transformer_latent_diffusion_amd import _lib, schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = (t.to(_dev()).contiguous() for t in _inputs(2, seed=36))
    mask = _rect_masks(2).to(_dev()).contiguous() if entry == "from_mask" else None
    k, levels = schedule.truncate_levels(schedule.noise_schedule(8, 1), 1.0 if entry == "plain" else 0.65)
    co = np.ascontiguousarray(schedule.step_coefficients(levels), dtype=np.float32)
    nl, n = co.shape[0], eps.numel()
    assert (k == 0) == (entry == "plain") and nl >= 3
    h = m._ensure_engine(4, _dev())
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    cop, stream = co.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)

    def call(out, tx0):
        if entry == "plain":
            return _lib.lib().tld_sample(h, vp(eps), vp(labels), cop, nl, 3.0, 0.1, 0.1, vp(out), 2, vp(tx0), None, stream)
        return _lib.lib().tld_sample_from(h, vp(eps), vp(z0), vp(mask), float(np.float32(levels[0])), vp(labels), cop, nl, 3.0, 0.1, 0.1, vp(out), 2,
                                          vp(tx0), None, stream)

    out_a, tr_a = torch.empty_like(eps), torch.zeros((nl - 1,) + tuple(eps.shape), device=_dev())
    buf_o, buf_t = torch.zeros(n + 4, device=_dev()), torch.zeros((nl - 1) * n + 4, device=_dev())
    out_u, tr_u = buf_o[1:1 + n].view_as(eps), buf_t[1:1 + (nl - 1) * n].view(nl - 1, *eps.shape)
    assert out_u.data_ptr() % 16 == 4 and tr_u.data_ptr() % 16 == 4
    assert call(out_a, tr_a) == 0 and call(out_u, tr_u) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out_a).all() and tr_a.abs().sum() > 0
    assert torch.equal(out_a, out_u) and torch.equal(tr_a, tr_u), "the scalar instantiation differs from the 16-byte one"
    assert float(buf_o[0]) == 0.0 and float(buf_o[-3:].abs().max()) == 0.0 and float(buf_t[0]) == 0.0 and float(buf_t[-3:].abs().max()) == 0.0


# ---- the known region --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_known_region_is_kept_exactly(plus):
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(3)
    mask = _rect_masks(3)
    lat, tx0, txt = gen.generate_latents_from(z0, labels, strength=0.65, mask=mask, n_iter=8, class_guidance=3.0, seeds=eps,
                                              sharp_f=0, bright_f=0, use_ddpm_plus=plus, trace=True)
    lat, txt = lat.cpu(), txt.cpu()
    keep = (mask == 0).expand_as(lat)
    assert keep.any() and (~keep).any()
    assert torch.equal(lat[keep], z0[keep]), "the kept region of the end latent is not the initial latent"
    assert not torch.equal(lat[~keep], z0[~keep])
    k, levels = schedule.truncate_levels(schedule.noise_schedule(8, 1), 0.65)
    assert txt.shape[0] == len(levels) - 1
    worst = 0.0
    for i in range(len(levels) - 1):
        s = levels[i + 1]
        known = s * eps + (1 - s) * z0
        worst = max(worst, float((txt[i][keep] - known[keep]).abs().max()))
    print(f"known region of trace_xt: worst abs difference {worst:.3e}")
    assert worst <= 1e-6


# ---- parity against the reference loop ---------------------------------------------------------------------------------------------
def _parity(fixture, B, n_iter, strength, mask, plus, g, seed):
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(fixture)
    eps, z0, labels = _inputs(B, seed=seed)
    lat, tx0, txt = gen.generate_latents_from(z0, labels, strength=strength, mask=mask, n_iter=n_iter, class_guidance=g, seeds=eps,
                                              sharp_f=0.1, bright_f=0.1, use_ddpm_plus=plus, trace=True)
    k, levels = schedule.truncate_levels(schedule.noise_schedule(n_iter, 1), strength)
    s0 = float(np.float32(levels[0])) if k > 0 else 1.0
    ref = TorchRefDenoiser(asdict(cfg), sd)
    rlat, rx0, rxt = R.sample_from(ref, eps, z0, mask, labels, levels, s0, g, plus, 0.1, 0.1, trace=True)
    sel = torch.ones_like(lat.cpu(), dtype=torch.bool) if mask is None else (mask > 0).expand_as(rlat)
    e_lat = _rel_rms(lat.cpu(), rlat, sel)
    e_x0 = max(_rel_rms(tx0[i].cpu(), rx0[i], sel) for i in range(len(levels) - 1))
    e_xt = max(_rel_rms(txt[i].cpu(), rxt[i], sel) for i in range(len(levels) - 1))
    return k, len(levels), e_lat, e_x0, e_xt


def _hold(tag, k, n, e_lat, e_x0, e_xt):
    print(f"img2img parity {tag}: k={k}, {n} levels: end latent {e_lat:.3e}, worst-step trace_x0 {e_x0:.3e}, trace_xt {e_xt:.3e}")
    for what, e in (("end latent", e_lat), ("worst-step trace_x0", e_x0), ("worst-step trace_xt", e_xt)):
        assert np.isfinite(e) and e <= TRAJ_TOL, f"{tag}: {what} rel-rms {e:.3e} exceeds the contract tolerance {TRAJ_TOL:.1e}"


@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("strength", [0.65, 0.35])
def test_parity_tiny_vs_reference_loop(strength, masked, plus):
    mask = _rect_masks(2) if masked else None
    _hold(f"tiny s={strength} {'mask' if masked else 'nomask'} {'dpm' if plus else 'ddim'}",
          *_parity(TINY, 2, 8, strength, mask, plus, 3.0, seed=41))


def test_parity_tiny_fractional_mask_vs_reference_loop():
    _hold("tiny s=0.65 fractional mask dpm", *_parity(TINY, 2, 8, 0.65, _frac_mask(2), True, 3.0, seed=42))


def test_parity_100m_masked_vs_reference_loop():
    """The 100 M model at 32 x 32 latents, batch 2, n_iter = 6, strength 0.65, rectangle masks."""
    _hold("100m s=0.65 mask dpm", *_parity(BIG, 2, 6, 0.65, _rect_masks(2), True, 6.0, seed=43))


# ---- one launch per step -------------------------------------------------------------------------------------------------------------
def test_one_update_launch_per_step_with_a_mask():
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(2)
    kw = dict(strength=0.65, mask=_rect_masks(2), n_iter=8, class_guidance=3.0, seeds=eps)
    gen.generate_latents_from(z0, labels, **kw)                 # (builds the engine)
    k, levels = schedule.truncate_levels(schedule.noise_schedule(8, 1), 0.65)
    m.set_profile(["update"])
    try:
        gen.generate_latents_from(z0, labels, **kw)
        ms, n = m.get_profile("update")
    finally:
        m.set_profile([])
    assert n == len(levels) and ms > 0.0, (n, len(levels), ms)


# ---- end to end: picture in, picture out -----------------------------------------------------------------------------------------------
def test_image_to_image_all_native():
    """PIL image -> native VAE encoder -> tld_sample_from -> native VAE decoder -> PIL image, with synthetic weights (as
    test_text_to_image_all_native builds its pipeline); with a mask whose kept region covers whole 8 x 8 latent cells the returned
    latents there are the encoder's ``mode() / 8`` exactly."""
    from PIL import Image
    from transformer_latent_diffusion_amd import AutoencoderKL, DenoiserConfig, DiffusionTransformer, LTDConfig, latent_mask
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    from transformer_latent_diffusion_amd.vae import VaeDecoderConfig
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(_dev())
    vae = AutoencoderKL(VaeEncoderConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1),
                        VaeDecoderConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1), init_seed=3, max_batch=2).to(_dev())

    def tokenize(prompts):                               # clip.tokenize stand-in: SOT, one id per character, EOT, zero padding
        t = torch.zeros(len(prompts), ccfg.context_length, dtype=torch.long)
        for i, p in enumerate(prompts):
            ids = [1 + (ord(ch) % 900) for ch in p][: ccfg.context_length - 2]
            t[i, 0] = ccfg.vocab_size - 2
            t[i, 1:1 + len(ids)] = torch.tensor(ids)
            t[i, 1 + len(ids)] = ccfg.vocab_size - 1
        return t

    class Tok:
        def tokenize(self, prompts, truncate=True):
            return tokenize(prompts)

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=vae, clip_model=enc, tokenizer=Tok(),
                                run_device=_dev())
    size = pipe.diffuser.model.image_size                # 16 x 16 latents <- 128 x 128 pixels
    px = 8 * size
    img_t = torch.rand(3, px, px, generator=torch.Generator().manual_seed(5))
    pil_in = Image.fromarray((img_t.permute(1, 2, 0).numpy() * 255).astype(np.uint8))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)     # (the encoder warns that no checkpoint was loaded)
        a = pipe.generate_image_from_image(pil_in, "a cute cat", strength=0.6, seed=3, n_iter=6)
        assert isinstance(a, Image.Image) and a.size == (px, px) and a.mode == "RGB"
        b = pipe.generate_image_from_image(pil_in, "a cute cat", strength=0.6, seed=3, n_iter=6)
        c = pipe.generate_image_from_image(pil_in, "a cute cat", strength=0.6, seed=4, n_iter=6)
        assert np.array_equal(np.asarray(a), np.asarray(b)) and not np.array_equal(np.asarray(a), np.asarray(c))
        # inpainting: regenerate the left half and an extra strip that cuts through latent cells
        mask = torch.zeros(px, px)
        mask[:, : px // 2] = 1
        mask[40:44, px // 2: px // 2 + 20] = 1
        pic, lat = pipe.generate_image_from_image(img_t, "a cute cat", strength=0.6, mask=mask, seed=3, n_iter=6, return_latents=True)
        z0 = vae.encode((img_t.to(_dev()) * 2 - 1).unsqueeze(0)).latent_dist.mode() / 8
        pil_mask = Image.fromarray((mask.numpy() * 255).astype(np.uint8), mode="L")
        pic2 = pipe.generate_image_from_image(img_t, "a cute cat", strength=0.6, mask=pil_mask, seed=3, n_iter=6)
        s = pipe.generate_image_from_image(img_t, "a cute cat", strength=0.6, seed=3, n_iter=6, sample_posterior=True)
    assert isinstance(pic, Image.Image) and pic.size == (px, px) and lat.shape == (1, 4, size, size)
    assert np.array_equal(np.asarray(pic), np.asarray(pic2)), "a PIL mask and the same mask as a tensor give different pictures"
    assert isinstance(s, Image.Image) and s.size == (px, px)
    keep = (latent_mask(mask, size) == 0).unsqueeze(0).expand(1, 4, size, size)
    assert int(keep.sum()) == 4 * (size * (size // 2) - 3) and (~keep).any()       # the strip touches three cells of one latent row
    assert torch.equal(lat.cpu()[keep], z0.cpu()[keep]), "kept latent cells are not encode(image).mode() / 8"
    assert not torch.equal(lat.cpu()[~keep], z0.cpu()[~keep])
    for bad in (torch.rand(3, px, px + 8), torch.rand(1, px, px), torch.rand(3, px // 2, px // 2), torch.rand(3, px, px) + 1.0, "cat.png"):
        with pytest.raises(ValueError):
            pipe.generate_image_from_image(bad, "a cute cat")
    with pytest.raises(ValueError):
        pipe.generate_image_from_image(img_t, "a cute cat", mask=torch.zeros(px // 2, px // 2))

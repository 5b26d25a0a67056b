"""GPU: B independent requests in one sampler call (tld_sample_requests).

The defining rule is bitwise: request b of a mixed call -- its own guidance scale, schedule (levels and their number), negative label,
image-to-image strength and mask -- gets what the existing entry points return for that request alone.  Against the CPU reference loop
(tests/requests_ref.py) the trajectories with real negative labels are held to the project's contract tolerance (TRAJ_TOL = 6e-2; the first
combined prediction to the forward contract 2e-2).  Every test prints the figures it asserts."""
import ctypes as C
from dataclasses import asdict

import numpy as np
import pytest
import torch

import requests_ref as R
from conftest import cfg_from_arr, load_golden, synth_weights

pytestmark = pytest.mark.gpu

TRAJ_TOL = 6e-2          # the contract tolerance of a multi-step CFG trajectory (tests/test_gpu_parity.py)
FWD_TOL = 2e-2           # ... of one forward

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

# the five requests of the defining test: guidance, n_iter, one DDIM request, one with exponent 2
FIVE = dict(class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], n_iter=[8, 5, 8, 3, 5], use_ddpm_plus=[True, True, False, True, True],
            exponent=[1, 1, 1, 1, 2])


def _inputs(B, S=32, seed=61):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S, S, generator=gen)
    z0 = torch.randn(B, 4, S, S, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


def _rect_mask(S=32):
    m = torch.zeros(1, S, S)
    m[:, 5:21, 3:17] = 1
    return m


def _frac_mask(S=32):
    ramp = torch.clamp((torch.arange(S, dtype=torch.float32) - 4) / 8, 0, 1)
    ramp = torch.minimum(ramp, ramp.flip(0))
    return (ramp[:, None] * ramp[None, :]).unsqueeze(0).contiguous()


def _solo(gen, eps, labels, b, kw, sharp=0.1, bright=0.1):
    """request b alone through the existing entry point: (end latent [C,S,S], trace_x0 [n-1,C,S,S], trace_xt)"""
    lat, tx0, txt = gen.generate_latents(labels[b:b + 1], n_iter=kw["n_iter"][b], num_imgs=1, class_guidance=kw["class_guidance"][b], img_size=32,
                                         sharp_f=sharp, bright_f=bright, exponent=kw["exponent"][b], seeds=eps[b:b + 1],
                                         use_ddpm_plus=kw["use_ddpm_plus"][b], trace=True)
    return lat[0], tx0[:, 0], txt[:, 0]


def _hold_solo_equality(gen, eps, labels, kw, tag):
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, **kw)
    B = labels.shape[0]
    assert torch.isfinite(lat).all() and tx0.shape[0] == max(kw["n_iter"]) - 1 and tx0.shape[1] == B
    for b in range(B):
        a, ax0, axt = _solo(gen, eps, labels, b, kw)
        n = ax0.shape[0]
        assert n == kw["n_iter"][b] - 1
        assert torch.equal(lat[b], a), f"{tag}: end latent of request {b} differs from the request alone"
        assert torch.equal(tx0[:n, b], ax0), f"{tag}: trace_x0 of request {b} differs from the request alone"
        assert torch.equal(txt[:n, b], axt), f"{tag}: trace_xt of request {b} differs from the request alone"
        assert not tx0[n:, b].any() and not txt[n:, b].any(), f"{tag}: request {b} wrote a trace slot after it had finished"
    print(f"{tag}: {B} requests, levels {kw['n_iter']}: every end latent and trace slice bitwise equal to the solo call")
    return lat, tx0, txt


# ---- 1. solo equality, bitwise -------------------------------------------------------------------------------------------------------
def test_solo_equality_tiny_five_requests():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    _hold_solo_equality(gen, eps, labels, FIVE, "tiny")


BIG3 = dict(class_guidance=[6.0, 3.0, 4.5], n_iter=[4, 6, 6], use_ddpm_plus=[True, True, False], exponent=[1, 1, 2])


def test_solo_equality_100m_three_requests():
    """d = 768 at 256 tokens: the fused QKV -> attention kernel, the LayerNorm folds and CFG layer-0 sharing over a shrinking prefix."""
    cfg, sd, m, gen = _model(BIG)
    eps, z0, labels = _inputs(3, seed=62)
    _hold_solo_equality(gen, eps, labels, BIG3, "100m")


@pytest.mark.parametrize("cls,B", [(1, 3), (2, 2)], ids=["class1", "class2"])
def test_solo_equality_low_latency_classes(cls, B):
    cfg, sd, m, gen = _model(BIG, low_latency=cls)
    eps, z0, labels = _inputs(B, seed=63)
    kw = {k: v[:B] for k, v in BIG3.items()}
    _hold_solo_equality(gen, eps, labels, kw, f"100m low-latency class {cls}")


def _direct_call(m, eps, labels, coeffs, guid, out, tx0=None):
    """tld_sample_requests straight through ctypes on the caller's device tensors (records already in engine order)."""
    from transformer_latent_diffusion_amd import _lib
    B, n_max = eps.shape[0], coeffs[0].shape[0]
    table = np.zeros((B, n_max, 6), dtype=np.float32)
    recs = (_lib.TldSampleRequest * B)()
    for b in range(B):
        table[b, :coeffs[b].shape[0]] = coeffs[b]
        recs[b] = _lib.TldSampleRequest(coeffs[b].shape[0], guid[b], 1.0, 0)
    h = m._ensure_engine(2 * B, _dev())
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    rc = _lib.lib().tld_sample_requests(h, vp(eps), None, None, vp(labels), None, recs, table.ctypes.data_as(C.POINTER(C.c_float)), n_max, 0.1, 0.1,
                                        vp(out), B, vp(tx0), None, C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))
    return rc


def test_scalar_instantiation_through_an_odd_offset_view():
    """From Python every tensor is 16-byte aligned and C S S is a multiple of 16 (the token grid's side is a multiple of 4), so the
    16-byte instantiation is the only one the public interface can reach.  The scalar one (sampler_step_kernel<MASK, 1>) is reached
    here by handing the C ABI an out_latent and a trace_x0 that start 4 bytes into their buffers: same bits as the aligned call."""
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(3, seed=64)
    eps, labels = eps.to(_dev()).contiguous(), labels.to(_dev()).contiguous()
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1)) for n in (6, 4, 3)]
    guid = [3.0, 4.5, 1.5]
    n = eps.numel()
    out_a, tr_a = torch.empty_like(eps), torch.zeros((5,) + tuple(eps.shape), device=_dev())
    buf_o, buf_t = torch.zeros(n + 4, device=_dev()), torch.zeros(5 * n + 4, device=_dev())
    out_u, tr_u = buf_o[1:1 + n].view_as(eps), buf_t[1:1 + 5 * n].view(5, *eps.shape)
    assert out_u.data_ptr() % 16 == 4 and tr_u.data_ptr() % 16 == 4
    assert _direct_call(m, eps, labels, coeffs, guid, out_a, tr_a) == 0
    assert _direct_call(m, eps, labels, coeffs, guid, out_u, tr_u) == 0
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_u) and torch.equal(tr_a, tr_u), "the scalar instantiation differs from the 16-byte one"
    assert float(buf_o[0]) == 0.0 and float(buf_o[-3:].abs().max()) == 0.0 and float(buf_t[0]) == 0.0 and float(buf_t[-3:].abs().max()) == 0.0
    want = gen.generate_latents(labels[1:2], n_iter=4, num_imgs=1, class_guidance=4.5, img_size=32, sharp_f=0.1, bright_f=0.1, seeds=eps[1:2])
    assert torch.equal(out_u[1], want[0])


# ---- 2. a uniform call is the old call --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_uniform_call_is_generate_latents(plus):
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    kw = dict(n_iter=8, class_guidance=3.0, img_size=32, sharp_f=0.1, bright_f=0.1, seeds=eps, use_ddpm_plus=plus, trace=True)
    want = gen.generate_latents(labels, num_imgs=5, **kw)
    got = gen.generate_latents_requests(labels, **kw)
    for a, b, what in zip(got, want, ("end latent", "trace_x0", "trace_xt")):
        assert a.shape == b.shape and torch.equal(a, b), f"{what} differs from generate_latents"


# ---- 3. image-to-image mix ----------------------------------------------------------------------------------------------------------------
def test_image_to_image_mix_in_one_call():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(4, seed=65)
    strength = [None, 0.65, 0.65, 1.0]
    masks = [None, None, _rect_mask(), _frac_mask()]
    kw = dict(n_iter=8, class_guidance=3.0, sharp_f=0.1, bright_f=0.1)
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, init_latents=[None, z0[1], z0[2], z0[3]], strength=strength, mask=masks,
                                                  trace=True, **kw)
    levels_seen = []
    for b in range(4):
        s = slice(b, b + 1)
        if strength[b] is None:
            a = gen.generate_latents(labels[s], num_imgs=1, img_size=32, seeds=eps[s], trace=True, **kw)
        else:
            a = gen.generate_latents_from(z0[s], labels[s], strength=strength[b], mask=None if masks[b] is None else masks[b].unsqueeze(0),
                                          seeds=eps[s], trace=True, **kw)
        n = a[1].shape[0]
        assert torch.equal(lat[b], a[0][0]) and torch.equal(tx0[:n, b], a[1][:, 0]) and torch.equal(txt[:n, b], a[2][:, 0]), \
            f"request {b} (strength {strength[b]}, {'mask' if masks[b] is not None else 'no mask'}) differs from the request alone"
        levels_seen.append(n + 1)
    print(f"image-to-image mix: levels per request {levels_seen}; all four bitwise equal to their solo calls")
    assert levels_seen == [8, 5, 5, 8]
    # the kept region of the masked ones is z0 exactly (without the latent shifts, which move channels 0 and 3 everywhere)
    lat0 = gen.generate_latents_requests(labels, seeds=eps, init_latents=[None, z0[1], z0[2], z0[3]], strength=strength, mask=masks,
                                         n_iter=8, class_guidance=3.0, sharp_f=0, bright_f=0).cpu()
    for b in (2, 3):
        keep = (masks[b] == 0).expand(4, 32, 32)
        assert keep.any() and torch.equal(lat0[b][keep], z0[b][keep]), f"request {b}: the kept region is not the initial latent"
        assert not torch.equal(lat0[b][~keep], z0[b][~keep])


# ---- 4. negative labels -------------------------------------------------------------------------------------------------------------------
def test_zero_negative_labels_are_none():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    a = gen.generate_latents_requests(labels, seeds=eps, trace=True, **FIVE)
    b = gen.generate_latents_requests(labels, seeds=eps, negative_labels=torch.zeros(5, 768), trace=True, **FIVE)
    c = gen.generate_latents_requests(labels, seeds=eps, negative_labels=[None, torch.zeros(768), None, torch.zeros(768), None], trace=True, **FIVE)
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)


def _ulps(a, b):
    """distance in fp32 units in the last place, element by element (monotone integer image of the floats)"""
    def key(t):
        i = t.contiguous().view(torch.int32).to(torch.int64)
        return torch.where(i < 0, -(i & 0x7FFFFFFF), i)
    return (key(a) - key(b)).abs()


@pytest.mark.parametrize("fixture", [TINY, BIG], ids=["tiny", "100m"])
def test_negative_label_combines_the_two_predictions(fixture):
    """x0 = fma(g, f(label A), (1 - g) f(label B)) with the negative label B in the unconditional half: fA, fB are the first predictions
    of g = 1 calls (fma(1, f, 0 * unc) = f exactly); float32(float64(g) fA + float32((1 - g) fB)) recomputes the fma with a double
    rounding, hence 0 or 1 ulp."""
    cfg, sd, m, gen = _model(fixture)
    eps, z0, labels = _inputs(2, seed=66)
    A, Bl = labels[0:1], labels[1:2]
    x = eps[0:1]
    kw = dict(n_iter=2, seeds=x, sharp_f=0, bright_f=0, trace=True)
    fA = gen.generate_latents_requests(A, class_guidance=1.0, **kw)[1][0, 0].cpu()
    fB = gen.generate_latents_requests(Bl, class_guidance=1.0, **kw)[1][0, 0].cpu()
    g = 4.5
    got = gen.generate_latents_requests(A, class_guidance=g, negative_labels=Bl, **kw)[1][0, 0].cpu()
    one_minus_g = np.float32(1.0) - np.float32(g)
    t = (fB.numpy() * one_minus_g).astype(np.float32)
    want = torch.from_numpy((np.float64(g) * fA.numpy().astype(np.float64) + t.astype(np.float64)).astype(np.float32))
    u = _ulps(got, want)
    n1 = int((u == 1).sum())
    print(f"negative label, first combined prediction: {int((u == 0).sum())} elements at 0 ulp, {n1} at 1 ulp, worst {int(u.max())} ulp")
    assert int(u.max()) <= 1
    assert not torch.equal(got, gen.generate_latents_requests(A, class_guidance=g, **kw)[1][0, 0].cpu())     # the negative label is read


def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


@pytest.mark.parametrize("fixture,n_iter", [(TINY, [8, 5]), (BIG, [6, 4])], ids=["tiny", "100m"])
def test_trajectory_with_negative_labels_vs_reference_loop(fixture, n_iter):
    """Tiny 8 / 5 levels, 100 M 6 / 4 levels, batch 2, guidance 3.0 / 4.5, real negative labels, against tests/requests_ref.py: the contract
    tolerances, no regression bound (the figures are printed)."""
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(fixture)
    eps, z0, labels = _inputs(2, seed=67)
    neg = torch.randn(2, 768, generator=torch.Generator().manual_seed(68)) * 0.5
    g = [3.0, 4.5]
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, n_iter=n_iter, class_guidance=g, negative_labels=neg, sharp_f=0.1, bright_f=0.1,
                                                  trace=True)
    ref = TorchRefDenoiser(asdict(cfg), sd)
    levels = [schedule.noise_schedule(n, 1) for n in n_iter]
    rlat, rx0, rxt = R.sample_requests(ref, eps, None, None, labels, [neg[0], neg[1]], levels, [1.0, 1.0], g, [True, True], 0.1, 0.1, trace=True)
    lat, tx0, txt = lat.cpu(), tx0.cpu(), txt.cpu()
    for b in range(2):
        n = n_iter[b] - 1
        e_first = _rel_rms(tx0[0, b], rx0[0, b])
        e_lat = _rel_rms(lat[b], rlat[b])
        e_x0 = max(_rel_rms(tx0[i, b], rx0[i, b]) for i in range(n))
        e_xt = max(_rel_rms(txt[i, b], rxt[i, b]) for i in range(n))
        print(f"negative-label trajectory {fixture} request {b} (g {g[b]}, {n_iter[b]} levels): first combined prediction {e_first:.3e}, end latent "
              f"{e_lat:.3e}, worst-step trace_x0 {e_x0:.3e}, trace_xt {e_xt:.3e}")
        assert np.isfinite(e_first) and e_first <= FWD_TOL
        for e in (e_lat, e_x0, e_xt):
            assert np.isfinite(e) and e <= TRAJ_TOL


# ---- 5. / 6. order independence, repeatability ----------------------------------------------------------------------------------------------
def test_order_independence_and_repeatability():
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    neg = [None, labels[0] * 0.5, None, None, labels[2] * -1.0]
    first = gen.generate_latents_requests(labels, seeds=eps, negative_labels=neg, trace=True, **FIVE)
    perm = [3, 0, 4, 2, 1]
    kw = {k: [v[i] for i in perm] for k, v in FIVE.items()}
    second = gen.generate_latents_requests(labels[perm], seeds=eps[perm], negative_labels=[neg[i] for i in perm], trace=True, **kw)
    for u, v in zip(first, second):
        idx = (slice(None), perm) if u.dim() == 5 else (perm,)
        assert torch.equal(u[idx], v), "a request's result depends on the order of submission"
    gen.generate_latents(labels[:2], n_iter=6, num_imgs=2, class_guidance=2.0, img_size=32, seeds=eps[:2])      # an intervening plain call
    third = gen.generate_latents_requests(labels, seeds=eps, negative_labels=neg, trace=True, **FIVE)
    again = gen.generate_latents_requests(labels, seeds=eps, negative_labels=neg, trace=True, **FIVE)
    for u, v, w in zip(first, third, again):
        assert torch.equal(u, v) and torch.equal(u, w), "two identical calls differ"


# ---- 7. launch accounting ---------------------------------------------------------------------------------------------------------------------
def test_launch_accounting_and_path_bits():
    from transformer_latent_diffusion_amd import Denoiser
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    want = gen.generate_latents_requests(labels, seeds=eps, **FIVE)               # (builds the engine)
    m.set_profile(["update"])
    try:
        gen.generate_latents_requests(labels, seeds=eps, **FIVE)
        ms, n = m.get_profile("update")
    finally:
        m.set_profile([])
    assert n == max(FIVE["n_iter"]) and ms > 0.0, (n, ms)                         # one launch per step over the active prefix
    names = Denoiser.SAMPLER_PATH_NAMES
    old = sum(1 << i for i, nm in enumerate(Denoiser.PATH_NAMES) if nm in ("update", "update_from", "update_from masked", "start_mix"))
    new = sum(1 << i for i in names)
    bit = {v: k for k, v in names.items()}
    m.set_debug(True)
    try:
        got = gen.generate_latents_requests(labels, seeds=eps, **FIVE)
        p_plain = m.debug_paths()
        gen.generate_latents_requests(labels, seeds=eps, init_latents=z0, strength=[None, 0.65, None, None, 0.7], **FIVE)
        p_mix = m.debug_paths()
        gen.generate_latents_requests(labels, seeds=eps, init_latents=z0, strength=[None, 0.65, None, None, 0.7],
                                      mask=[None, _rect_mask(), None, None, None], **FIVE)
        p_mask = m.debug_paths()
        with pytest.raises(RuntimeError, match="status 2"):                       # the entry keeps no stage
            m.read_stage("step.x0")
        gen.generate_latents(labels, n_iter=4, num_imgs=5, class_guidance=3.0, img_size=32, seeds=eps)
        p_old = m.debug_paths()
    finally:
        m.set_debug(False)
    assert torch.equal(got, want), "a debug call computes something else"
    print(f"launch paths: requests {p_plain:#x}, with a start mix {p_mix:#x}, with a mask {p_mask:#x}, generate_latents afterwards {p_old:#x}")
    assert p_plain & new == 1 << bit["update_requests"] and not p_plain & old
    assert p_mix & new == (1 << bit["update_requests"]) | (1 << bit["start_mix per request"]) and not p_mix & old
    assert p_mask & new == (1 << bit["update_requests masked"]) | (1 << bit["start_mix per request"]) and not p_mask & old
    assert p_old & old == 1 << Denoiser.PATH_NAMES.index("update") and not p_old & new


# ---- 8. the pipeline ----------------------------------------------------------------------------------------------------------------------------
def test_pipeline_per_prompt_scalars_and_mixed_batcher():
    from PIL import Image
    from transformer_latent_diffusion_amd import (AutoencoderKLDecoder, DenoiserConfig, DiffusionTransformer, LTDConfig, RequestBatcher,
                                                  VaeDecoderConfig)
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(_dev())
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2).to(_dev())

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

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=vae, clip_model=enc, tokenizer=Tok(), run_device=_dev())
    prompts, guid, n_it, seeds = ["a cute cat", "a red car", "a tall tree", "a cute cat"], [6.0, 3.0, 4.5, 6.0], [4, 6, 4, 5], [3, 4, 5, 6]
    pics = pipe.generate_images_from_texts(prompts, class_guidance=guid, seeds=seeds, n_iter=n_it)
    assert len(pics) == 4 and all(isinstance(p, Image.Image) for p in pics)
    for i in range(4):
        alone = pipe.generate_image_from_text(prompts[i], class_guidance=guid[i], seed=seeds[i], n_iter=n_it[i])
        assert np.array_equal(np.asarray(pics[i]), np.asarray(alone)), f"prompt {i}: the mixed call's picture differs from the one-prompt call"
    # a negative prompt changes the picture, repeats, and the batched negative equals the one-prompt negative
    neg = pipe.generate_images_from_texts(prompts[:2], class_guidance=guid[:2], seeds=seeds[:2], n_iter=n_it[:2], negative_prompts=["blurry", None])
    assert not np.array_equal(np.asarray(neg[0]), np.asarray(pics[0])) and np.array_equal(np.asarray(neg[1]), np.asarray(pics[1]))
    one = pipe.generate_image_from_text(prompts[0], class_guidance=guid[0], seed=seeds[0], n_iter=n_it[0], negative_prompt="blurry")
    assert np.array_equal(np.asarray(one), np.asarray(neg[0]))

    # RequestBatcher: the same queue, grouped (one sampler call per (guidance, n_iter) pair) and mixed (one call)
    calls = []
    inner = pipe.diffuser.model.sample_latents_requests
    inner_old = pipe.diffuser.model.sample_latents
    pipe.diffuser.model.sample_latents_requests = lambda *a, **k: (calls.append("requests"), inner(*a, **k))[1]
    pipe.diffuser.model.sample_latents = lambda *a, **k: (calls.append("plain"), inner_old(*a, **k))[1]
    try:
        out = {}
        for mixed in (False, True):
            rb = RequestBatcher(pipe, max_batch=8, mixed=mixed)
            tickets = [rb.submit(p, g, s, n) for p, g, s, n in zip(prompts, guid, seeds, n_it)]
            calls.clear()
            res = rb.flush()
            out[mixed] = ([res[t] for t in tickets], list(calls))
    finally:
        del pipe.diffuser.model.sample_latents_requests, pipe.diffuser.model.sample_latents
    assert out[False][1] == ["plain"] * 4 and out[True][1] == ["requests"], out
    for a, b in zip(out[False][0], out[True][0]):
        assert np.array_equal(np.asarray(a), np.asarray(b)), "the mixed batcher's picture differs from the grouped batcher's"


# ---- 9. refusals on the device side ----------------------------------------------------------------------------------------------------------------
def test_device_side_refusals_enqueue_nothing():
    from transformer_latent_diffusion_amd import _lib, schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    want = gen.generate_latents_requests(labels, seeds=eps, **FIVE)
    L = _lib.lib()
    h = m._engine
    cap = m._engine_batch
    dev = _dev()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(B, recs, n_max, table, noise, init=None, mask=None, lab=None, out=None):
        arr = (_lib.TldSampleRequest * B)(*recs)
        vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
        rc = L.tld_sample_requests(h, vp(noise), vp(init), vp(mask), vp(lab), None, arr, table.ctypes.data_as(C.POINTER(C.c_float)), n_max, 0.0, 0.0,
                                   vp(out), B, None, None, stream)
        return rc, L.tld_last_error().decode()

    co4 = schedule.step_coefficients(schedule.noise_schedule(4, 1))
    Rq = _lib.TldSampleRequest
    # 2 B > max_batch
    Bbig = cap // 2 + 1
    big = torch.zeros(Bbig, 4, 32, 32, device=dev)
    rc, msg = call(Bbig, [Rq(4, 3.0, 1.0, 0)] * Bbig, 4, np.tile(co4, (Bbig, 1, 1)), big, lab=torch.zeros(Bbig, 768, device=dev), out=torch.empty_like(big))
    assert rc == 1 and "max_batch" in msg, (rc, msg)
    # more than 1024 conditioning rows: 4 requests of 300 pairwise distinct levels each
    n = 300
    tab = np.zeros((4, n, 6), dtype=np.float32)
    for b in range(4):
        lv = [0.99 - 1e-4 * (4 * i + b) for i in range(n)]
        tab[b] = schedule.step_coefficients(lv)
    x4 = eps[:4].to(dev).contiguous()
    sentinel = torch.full_like(x4, 7.0)
    rc, msg = call(4, [Rq(n, 3.0, 1.0, 0)] * 4, n, tab, x4, lab=labels[:4].to(dev).contiguous(), out=sentinel)
    assert rc == 1 and "1205" in msg and "1024" in msg, (rc, msg)          # 4 x 300 sigmas + 4 labels + the zero row
    # start_mix outside (0, 1], and a mask without init_latent
    tab4 = np.tile(co4, (4, 1, 1))
    for bad in (0.0, 1.5, -0.2):
        rc, msg = call(4, [Rq(4, 3.0, 1.0, 0), Rq(4, 3.0, bad, 0)] + [Rq(4, 3.0, 1.0, 0)] * 2, 4, tab4, x4, init=x4, lab=labels[:4].to(dev).contiguous(),
                       out=sentinel)
        assert rc == 1 and "start_mix" in msg and "request 1" in msg, (rc, msg)
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, mask=torch.ones(4, 1, 32, 32, device=dev), lab=labels[:4].to(dev).contiguous(), out=sentinel)
    assert rc == 1 and "init_latent" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()), "a refused call wrote its output"
    # a following valid call is bitwise right
    assert torch.equal(gen.generate_latents_requests(labels, seeds=eps, **FIVE), want)

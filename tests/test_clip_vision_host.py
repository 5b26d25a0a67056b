"""CPU: the CLIP image tower's float64 restatement, key handling, preprocessing, score and the refusals that need no device.

The GPU tests (tests/test_gpu_clip_vision_stages.py, tests/test_gpu_clip_vision.py) compare the engine with tests/clip_vision_refs.py; this file
pins that restatement to transformers' CLIPVisionModelWithProjection (random weights through ``clip_visual_from_transformers``) at the bound
tests/test_clip_stage_refs_host.py uses for the text chain, and holds everything else that needs no device.

The attention yardstick (test_attention_model_against_exact): the relative rms between ``attention_model`` (clip_vis_attn_kernel's documented
roundings) and ``attention_exact`` on the GPU cases' inputs (two heads, three samples), n = 2 ... 257: random 1.81e-3 ... 2.21e-3, negative
1.70e-3 ... 2.13e-3, tail-peaked 1.46e-3 ... 1.83e-3 and class-peaked 1.37e-3 ... 1.72e-3 from n = 5 on -- one bf16 rounding of the output plus
the rounding of P -- and 6.6e-4 / 4.2e-4 for the two peaked kinds at n = 2, where P is nearly (0, 1) and the class-peaked value is below the
2^-11 under which the GPU test takes the ROUND bound instead.  The GPU test's bound is twice the yardstick, member by member.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import clip_vision_refs as V
from test_clip_host import TINY as TEXT_TINY
from test_clip_stage_refs_host import FP32_REF_TOL
from test_gemm_plan import EPI_BIAS_BF16, EPI_F32, FAMILY, MAIN, REFUSAL, plan
from transformer_latent_diffusion_amd import _lib
from transformer_latent_diffusion_amd.clip_image import (CLIP_MEAN, CLIP_STD, Clip, ClipImageEncoder, ClipVisionConfig, clip_preprocess, clip_score,
                                                         clip_visual_from_transformers, clip_visual_spec, synth_clip_visual_state_dict)
from transformer_latent_diffusion_amd.clip_text import ClipTextEncoder, synth_clip_state_dict

TLD_ERR_INVALID = 1


def vcfg(patch, g, width, layers=2, embed_dim=64):
    return ClipVisionConfig(image_size=patch * g, patch_size=patch, width=width, heads=width // 64, layers=layers, embed_dim=embed_dim)


# (patch, g) -> tokens 5, 17, 50, 65, 197, 257: contraction lengths 588 (padded to 640), 3072 and 768
GEOMETRY = {5: (14, 2), 17: (14, 4), 50: (32, 7), 65: (14, 8), 197: (16, 14), 257: (14, 16)}
# name: (config, batch, max_batch, weight seed) -- the GPU cases; batch is always below max_batch
CASES = {}
for _n in (5, 17, 50, 65):
    for _w in (64, 128):
        CASES[f"T{_n}W{_w}"] = (vcfg(*GEOMETRY[_n], _w), 3, 4, 10 + len(CASES))
for _n in (197, 257):
    CASES[f"T{_n}W128"] = (vcfg(*GEOMETRY[_n], 128), 3, 4, 10 + len(CASES))
CASES["WIDTH"] = (vcfg(14, 16, 1024, embed_dim=768), 2, 3, 30)
CASES["DEPTH"] = (vcfg(14, 16, 256, layers=24), 2, 3, 31)


def case_weights(name):
    cfg, _, _, seed = CASES[name]
    return {k: torch.from_numpy(v) for k, v in synth_clip_visual_state_dict(cfg, seed).items()}


def case_pixels(name, batch=None, seed=0):
    """Normalised-pixel-like input: unit normal, so every patch feature is O(1)."""
    cfg, b, _, s = CASES[name]
    g = torch.Generator().manual_seed(1000 + s + seed)
    return torch.randn(batch or b, 3, cfg.image_size, cfg.image_size, generator=g)


def _rel(a, b):
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


# ---- the float64 chain against transformers ---------------------------------------------------------------------------------------

def _hf_model(cfg, seed):
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    hc = CLIPVisionConfig(hidden_size=cfg.width, intermediate_size=4 * cfg.width, projection_dim=cfg.embed_dim, num_hidden_layers=cfg.layers,
                          num_attention_heads=cfg.heads, image_size=cfg.image_size, patch_size=cfg.patch_size, hidden_act="quick_gelu",
                          attn_implementation="eager")
    m = CLIPVisionModelWithProjection(hc).eval().float()
    with torch.no_grad():                          # transformers initialises biases to zero and LayerNorms to (1, 0): make every term count
        for k, p in m.named_parameters():
            if k.endswith("bias"):
                p.add_(0.1 * torch.randn_like(p))
            elif "norm" in k:
                p.add_(0.2 * torch.randn_like(p))
            else:
                p.mul_(3.0)
    return m


@pytest.mark.parametrize("patch,g,width", [(p, g, w) for p in (14, 16, 32) for g in (2, 4, 7) for w in (64, 128)])
def test_chain_against_transformers(patch, g, width):
    cfg = vcfg(patch, g, width, embed_dim=96)
    m = _hf_model(cfg, patch * 100 + g * 10 + width)
    sd = clip_visual_from_transformers(m.state_dict())
    assert {k: tuple(v.shape) for k, v in sd.items()} == dict(clip_visual_spec(cfg))
    pix = torch.randn(3, 3, cfg.image_size, cfg.image_size, generator=torch.Generator().manual_seed(g))
    with torch.no_grad():
        want = m(pixel_values=pix).image_embeds.double()
    got = V.chain(cfg, sd, pix)
    assert got.dtype == torch.float64 and got.shape == want.shape == (3, 96)
    assert _rel(got, want) < FP32_REF_TOL and float((got - want).abs().max()) < 1e-4 * max(1.0, float(want.abs().max()))


def test_rounded_chain_is_close_but_not_equal():
    cfg = CASES["T17W64"][0]
    w, pix = case_weights("T17W64"), case_pixels("T17W64")
    e = _rel(V.chain(cfg, w, pix, rounded=True), V.chain(cfg, w, pix))
    assert 1e-4 < e < 3e-2, e


# ---- key handling ----------------------------------------------------------------------------------------------------------------

def _full_clip_dict(cfg, tcfg=TEXT_TINY):
    sd = {k: torch.from_numpy(v) for k, v in synth_clip_state_dict(tcfg, 3).items()}
    sd.update({k: torch.from_numpy(v) for k, v in synth_clip_visual_state_dict(cfg, 4).items()})
    sd["logit_scale"] = torch.tensor(4.6)
    return sd


def test_spec_and_synth_agree():
    cfg = vcfg(14, 2, 128, layers=3)
    sd = synth_clip_visual_state_dict(cfg, 0)
    assert {k: v.shape for k, v in sd.items()} == dict(clip_visual_spec(cfg))
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in sd.values())
    again = synth_clip_visual_state_dict(cfg, 0)
    assert all(np.array_equal(sd[k], again[k]) for k in sd) and not np.array_equal(sd["visual.proj"], synth_clip_visual_state_dict(cfg, 1)["visual.proj"])
    assert ClipVisionConfig().tokens == 257 and dict(clip_visual_spec(ClipVisionConfig()))["visual.conv1.weight"] == (1024, 3, 14, 14)


@pytest.mark.parametrize("which", ["text TINY seed 3", "visual 14 2 64 seed 0", "visual 14 2 128 embed 768 seed 0"])
def test_synthetic_weights_are_pinned(which):
    """sha1 of every tensor (shape and fp32 bytes) of both towers' deterministic initialisation, as recorded in tests/golden/clip_synth_digests.json
    before the towers shared their spec and draw helpers: the draw order, dtypes and scales are part of every pinned GPU result."""
    import hashlib
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "clip_synth_digests.json")) as f:
        want = json.load(f)[which]
    sd = {"text TINY seed 3": lambda: synth_clip_state_dict(TEXT_TINY, 3), "visual 14 2 64 seed 0": lambda: synth_clip_visual_state_dict(vcfg(14, 2, 64), 0),
          "visual 14 2 128 embed 768 seed 0": lambda: synth_clip_visual_state_dict(vcfg(14, 2, 128, embed_dim=768), 0)}[which]()
    assert list(sd) == list(want)                                   # the same keys in the same order
    for k, v in sd.items():
        assert v.dtype == np.float32
        assert hashlib.sha1(repr(tuple(v.shape)).encode() + np.ascontiguousarray(v).tobytes()).hexdigest() == want[k], k


def test_full_clip_dict_loads_into_both_towers():
    cfg = vcfg(14, 2, 64)
    sd = _full_clip_dict(cfg)
    enc = ClipImageEncoder(cfg).load_state_dict(sd)
    assert torch.equal(enc.state_dict()["visual.proj"], sd["visual.proj"]) and set(enc.state_dict()) == set(clip_visual_spec(cfg))
    ClipTextEncoder(TEXT_TINY).load_state_dict(sd)                  # the text tower still takes the same dict
    both = Clip(ClipTextEncoder(TEXT_TINY), ClipImageEncoder(cfg)).load_state_dict(sd)
    assert both.visual.input_resolution == 28 and set(both.state_dict()) == set(sd) - {"logit_scale"}
    assert torch.equal(both.state_dict()["text_projection"], sd["text_projection"])


def test_bad_keys_raise():
    cfg = vcfg(14, 2, 64)
    sd = _full_clip_dict(cfg)
    missing = {k: v for k, v in sd.items() if k != "visual.ln_post.bias"}
    with pytest.raises(RuntimeError, match="missing keys in CLIP state_dict"):
        ClipImageEncoder(cfg).load_state_dict(missing)
    ClipImageEncoder(cfg).load_state_dict(missing, strict=False)
    with pytest.raises(RuntimeError, match="unexpected key 'visual.nonsense'"):
        ClipImageEncoder(cfg).load_state_dict(dict(sd, **{"visual.nonsense": torch.zeros(1)}))
    with pytest.raises(RuntimeError, match="unexpected key 'nonsense'"):
        Clip(ClipTextEncoder(TEXT_TINY), ClipImageEncoder(cfg)).load_state_dict(dict(sd, nonsense=torch.zeros(1)))
    with pytest.raises(RuntimeError, match="size mismatch for visual.class_embedding"):
        ClipImageEncoder(cfg).load_state_dict(dict(sd, **{"visual.class_embedding": torch.zeros(65)}))
    with pytest.raises(ValueError, match="head_dim must be 64"):
        ClipImageEncoder(ClipVisionConfig(width=128, heads=4))


def test_encode_image_refuses_what_it_cannot_take():
    enc = ClipImageEncoder(vcfg(14, 2, 64))
    with pytest.raises(ValueError, match=r"expected pixels \[B, 3, 28, 28\]"):
        enc.encode_image(torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
        enc.encode_image(torch.zeros(1, 3, 28, 28, dtype=torch.float64))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a HIP device"):
            enc.encode_image(torch.zeros(1, 3, 28, 28))


# ---- clip_preprocess ---------------------------------------------------------------------------------------------------------------

def test_preprocess_tensor_path():
    mean, std = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    assert CLIP_MEAN == (0.48145466, 0.4578275, 0.40821073) and CLIP_STD == (0.26862954, 0.26130258, 0.27577711)
    g = torch.Generator().manual_seed(0)
    x = torch.rand(2, 3, 32, 32, generator=g)
    assert torch.equal(clip_preprocess(x, 32), (x - mean) / std)                        # already at size: only normalised, bit for bit
    wide = torch.rand(2, 3, 48, 80, generator=g)
    y = clip_preprocess(wide, 32)
    assert y.shape == (2, 3, 32, 32) and y.dtype == torch.float32
    # the shorter side becomes 32 (80 -> 53 columns), then the centre 32 columns are kept: a marker left or right of the centre window is cropped away
    marked = torch.full((1, 3, 48, 80), 0.5)
    marked[..., :12] = 1.0
    marked[..., -12:] = 0.0
    flat = clip_preprocess(marked, 32)
    assert torch.allclose(flat, ((torch.full((1, 3, 32, 32), 0.5) - mean) / std), atol=1e-6)
    tall = torch.full((1, 3, 80, 48), 0.5)
    tall[..., 30:50, :] = 1.0                                                           # the centre rows survive
    out = clip_preprocess(tall, 32) * std + mean
    assert float(out[..., 12:20, :].min()) > 0.99 and abs(float(out[..., 0, :].mean()) - 0.5) < 1e-5
    lo, hi = (0 - mean) / std, (1 - mean) / std
    over = clip_preprocess(torch.rand(1, 3, 64, 64, generator=g).round(), 32)           # bicubic overshoot is clamped to [0, 1] before normalising
    assert bool((over >= lo - 1e-6).all()) and bool((over <= hi + 1e-6).all())
    with pytest.raises(ValueError, match="float tensor"):
        clip_preprocess(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), 8)


def test_preprocess_pil_path():
    from PIL import Image
    rng = np.random.default_rng(0)
    a = rng.integers(0, 256, (60, 90, 3), dtype=np.uint8)
    im = Image.fromarray(a)
    got = clip_preprocess(im, 32)
    # restated: Resize(32, BICUBIC) of the shorter side, CenterCrop(32), ToTensor, Normalize
    r = im.resize((int(32 * 90 / 60), 32), Image.BICUBIC)
    left = int(round((r.size[0] - 32) / 2.0))
    r = np.asarray(r.crop((left, 0, left + 32, 32)), dtype=np.float32) / 255.0
    want = (torch.from_numpy(r).permute(2, 0, 1) - torch.tensor(CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CLIP_STD).view(3, 1, 1)
    assert got.shape == (1, 3, 32, 32) and torch.equal(got[0], want)
    two = clip_preprocess([im, im.transpose(Image.ROTATE_90)], 32)
    assert two.shape == (2, 3, 32, 32) and torch.equal(two[0], got[0])
    same = clip_preprocess(Image.fromarray(a[:32, :32]), 32)                            # already at size: no resampling
    px = torch.from_numpy(a[:32, :32].astype(np.float32) / 255.0).permute(2, 0, 1)
    assert torch.equal(same[0], (px - torch.tensor(CLIP_MEAN).view(3, 1, 1)) / torch.tensor(CLIP_STD).view(3, 1, 1))


# ---- clip_score --------------------------------------------------------------------------------------------------------------------

def test_clip_score_against_numpy():
    rng = np.random.default_rng(1)
    a, b = rng.standard_normal((7, 48)).astype(np.float32), rng.standard_normal((7, 48)).astype(np.float32)
    a[2] = 0.0
    b[5] = 0.0
    got = clip_score(torch.from_numpy(a), torch.from_numpy(b))
    na, nb = np.linalg.norm(a.astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    want = np.where(na * nb > 0, (a.astype(np.float64) * b).sum(1) / np.maximum(na * nb, 1e-300), 0.0)
    assert got.dtype == torch.float32 and got.shape == (7,)
    assert float(got[2]) == 0.0 and float(got[5]) == 0.0 and bool(torch.isfinite(got).all())
    assert np.allclose(got.numpy(), want, atol=1e-6)
    assert float(clip_score(torch.from_numpy(a[:1]), torch.from_numpy(3 * a[:1]))[0]) == pytest.approx(1.0, abs=1e-6)
    half = clip_score(torch.from_numpy(a).half(), torch.from_numpy(b).half())
    assert half.dtype == torch.float32
    with pytest.raises(ValueError, match=r"two \[B, E\] tensors"):
        clip_score(torch.zeros(2, 3), torch.zeros(2, 4))


# ---- refusals without a device -------------------------------------------------------------------------------------------------------

GOOD = dict(image_size=224, patch_size=14, width=1024, heads=16, layers=24, embed_dim=768, max_batch=4, device_id=0)


@pytest.mark.parametrize("bad,reason", [
    (dict(width=1088, heads=17), b"a multiple of 64 in 64..1024"), (dict(width=96, heads=1), b"a multiple of 64 in 64..1024"),
    (dict(width=0, heads=0), b"a multiple of 64 in 64..1024"),
    (dict(heads=8), b"head_dim must be 64"),
    (dict(layers=0), b"layers=0: 1..64"), (dict(layers=65), b"layers=65: 1..64"),
    (dict(image_size=225), b"multiple of patch_size"), (dict(image_size=0), b"multiple of patch_size"),
    (dict(image_size=336), b"336 px towers (577 tokens) are out of scope"), (dict(image_size=238), b"at most 257 tokens"),
    (dict(patch_size=0), b"patch_size=0: 1..32"), (dict(patch_size=33, image_size=66), b"patch_size=33: 1..32"),
    (dict(embed_dim=0), b"must be positive"), (dict(max_batch=0), b"must be positive"),
])
def test_create_refuses_before_any_hip_call(bad, reason):
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.TldClipVisConfig(*dict(GOOD, **bad).values())
    assert L.tld_clip_vis_create(C.byref(cfg), C.byref(h)) == TLD_ERR_INVALID, bad
    assert h.value is None and reason in L.tld_last_error(), L.tld_last_error()


def test_null_arguments_of_every_entry():
    L = _lib.lib()
    h = C.c_void_p()
    cfg = _lib.TldClipVisConfig(*GOOD.values())
    buf = (C.c_float * 4)()
    shape = (C.c_int64 * 4)()
    one = C.c_void_p(C.addressof(buf))                        # a non-null pointer that is never dereferenced: the handle is checked first
    assert L.tld_clip_vis_create(None, C.byref(h)) == TLD_ERR_INVALID and L.tld_clip_vis_create(C.byref(cfg), None) == TLD_ERR_INVALID
    assert L.tld_clip_vis_load_tensor(None, b"visual.proj", one, shape, 1, 0) == TLD_ERR_INVALID
    assert L.tld_clip_vis_finalize_weights(None) == TLD_ERR_INVALID
    assert L.tld_clip_vis_encode_image(None, one, one, 1, 0, None) == TLD_ERR_INVALID and b"null" in L.tld_last_error()
    assert L.tld_clip_vis_set_debug(None, 1) == TLD_ERR_INVALID
    assert L.tld_clip_vis_read_stage(None, b"x0", buf, 4, shape) == TLD_ERR_INVALID
    assert L.tld_clip_vis_weight_bytes(None) == 0
    assert L.tld_clip_vis_destroy(None) == 0
    for args, reason in (((None, one, 1, 5, 1), b"null"), ((one, None, 1, 5, 1), b"null"), ((one, one, 0, 5, 1), b"batch=0"),
                         ((one, one, 1, 1, 1), b"n=1 tokens: 2..257"), ((one, one, 1, 258, 1), b"n=258 tokens: 2..257"),
                         ((one, one, 1, 5, 0), b"heads=0"), ((one, one, 1, 5, 17), b"heads=17")):
        assert L.tld_debug_clip_vis_attention(*args, None) == TLD_ERR_INVALID and reason in L.tld_last_error(), (args, L.tld_last_error())


# ---- the launch plans of the GPU cases -------------------------------------------------------------------------------------------------

def case_gemms(name):
    """(what, M, N, K, epilogue) of every GEMM launch of a case."""
    cfg, batch, _, _ = CASES[name]
    W, T, P = cfg.width, batch * cfg.tokens, batch * cfg.grid ** 2
    yield "conv1", P, W, V.padded_k(cfg.patch_size), EPI_F32
    yield "in_proj", T, 3 * W, W, EPI_BIAS_BF16
    yield "out_proj", T, W, W, EPI_F32
    yield "c_fc", T, 4 * W, W, EPI_BIAS_BF16
    yield "c_proj", T, W, 4 * W, EPI_F32


def test_every_gemm_of_the_cases_has_a_kernel():
    ks = set()
    for name in CASES:
        for what, M, N, K, epi in case_gemms(name):
            assert K % 64 == 0, (name, what, K)
            p = plan(M, N, K, epi, ncu=256)
            assert p[FAMILY] == MAIN and p[REFUSAL] == 0, (name, what, M, N, K, p)
            ks.add(K if what == "conv1" else None)
    assert {640, 3072, 768} <= ks                             # 588 padded, patch 32, patch 16
    # the shipped tower: ViT-L/14 at batch 16 and 64
    for B in (16, 64):
        for what, M, N, K, epi in (("conv1", B * 256, 1024, 640, EPI_F32), ("in_proj", B * 257, 3072, 1024, EPI_BIAS_BF16), ("out_proj", B * 257, 1024, 1024, EPI_F32),
                                   ("c_fc", B * 257, 4096, 1024, EPI_BIAS_BF16), ("c_proj", B * 257, 1024, 4096, EPI_F32)):
            assert plan(M, N, K, epi, ncu=256)[FAMILY] == MAIN, (B, what)


# ---- the attention yardstick ------------------------------------------------------------------------------------------------------------

ATTN_TOKENS = (2, 5, 17, 32, 33, 50, 64, 65, 197, 256, 257)       # the cases' counts, the tile edges around them and the smallest
ATTN_KINDS = ("random", "tail-peaked", "class-peaked", "negative")


def attention_inputs(n, heads, kind, batch=3, seed=0):
    """bf16-valued qkv rows [batch * n, 3 * 64 heads] (float32 holding bf16 values).
    random: unit normal q, k, v (scores of std 1).  tail-peaked / class-peaked: one key (n - 1 / 0) scores about +8 against every query while the others
    stay near 0, and its v row stands apart -- dropping or mis-masking it moves every output.  negative: every real score is about -98, so a row maximum
    taken over the zero scores of padded keys leaves e = exp(-98) = 0 in every real key."""
    g = torch.Generator().manual_seed(seed * 7919 + n * 31 + heads * 3 + ATTN_KINDS.index(kind))
    q, k, v = (torch.randn(batch, n, heads, 64, generator=g) for _ in range(3))
    u = torch.randn(batch, 1, heads, 64, generator=g)
    u = 8.0 * u / u.norm(dim=-1, keepdim=True)
    if kind in ("tail-peaked", "class-peaked"):
        j = n - 1 if kind == "tail-peaked" else 0
        q, k = u + 0.5 * q, 0.5 * k
        k[:, j] = u[:, 0] + 0.5 * torch.randn(batch, heads, 64, generator=g)
        v[:, j] += 3.0
    elif kind == "negative":
        q, k = 3.5 * u + 0.5 * q, -3.5 * u + 0.5 * k
    qkv = torch.cat([t.reshape(batch * n, heads * 64) for t in (q, k, v)], dim=1)
    return qkv.to(torch.bfloat16).to(torch.float32)


@pytest.mark.parametrize("kind", ATTN_KINDS)
def test_attention_model_against_exact(kind):
    """The yardstick of the GPU attention test: finite, non-zero and below one bf16 rounding's worst case (values: the module docstring)."""
    for n in ATTN_TOKENS:
        qkv = attention_inputs(n, 2, kind)
        exact, model = V.attention_exact(qkv, 3, n), V.attention_model(qkv, 3, n)
        assert bool(torch.isfinite(exact).all()) and bool(torch.isfinite(model).all())
        e = _rel(model, exact)
        assert 0.0 < e < 2.0 ** -8, (kind, n, e)           # below the worst case of one bf16 rounding per element
        if kind == "tail-peaked":                             # the peak is where it was put: the last key carries most of the weight
            without = V.attention_exact(torch.cat([qkv.view(3, n, -1)[:, :max(n - 1, 1)].reshape(-1, qkv.shape[1])]), 3, max(n - 1, 1))
            assert n == 2 or _rel(exact.view(3, n, -1)[:, :n - 1].reshape(without.shape), without) > 0.5

"""CPU: the host side of the device weight refresh -- the flat parameter vector (``weights.flatten_state_dict`` /
``weights.unflatten`` in ``train.param_layout`` order), ``Denoiser.load_flat`` without an engine, and the three new entries of the C ABI."""
import os
import shutil
import subprocess
from dataclasses import asdict

import numpy as np
import pytest
import torch

from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, _lib, flatten_state_dict, train, unflatten, weights

BUFFERS = ("fourier_feats.0.angular_speeds", "denoiser_trans_block.precomputed_pos_enc")
CONFIGS = {
    "d192_64tok": DenoiserConfig(image_size=16, noise_embed_dims=64, patch_size=2, embed_dim=192, dropout=0, n_layers=2, text_emb_size=32),
    "d128_patch4_3ch": DenoiserConfig(image_size=16, noise_embed_dims=32, patch_size=4, embed_dim=128, dropout=0, n_layers=3, text_emb_size=48, n_channels=3,
                                      mlp_multiplier=2),
    "d256_patch1": DenoiserConfig(image_size=8, noise_embed_dims=16, patch_size=1, embed_dim=256, dropout=0, n_layers=1, text_emb_size=768),
}


def _sd(cfg, seed):
    return {k: torch.from_numpy(np.array(v)) for k, v in weights.synth_state_dict(cfg, seed).items()}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_flatten_and_unflatten_round_trip_in_param_layout_order(name):
    cfg = CONFIGS[name]
    sd = _sd(cfg, 1)
    flat = flatten_state_dict(sd, cfg)
    lay = train.param_layout(cfg)
    assert flat.dtype == torch.float32 and flat.dim() == 1 and flat.numel() == weights.param_count(cfg)
    assert flat.numel() == sum(int(np.prod(s)) for _, s in lay.values())
    back = unflatten(flat, cfg)
    assert list(back) == list(lay) == [k for k in sd if k not in BUFFERS]              # the two buffers are not in the vector
    pos = 0
    for k, (off, shape) in lay.items():
        assert off == pos and tuple(back[k].shape) == shape
        assert torch.equal(back[k], sd[k]), k
        assert torch.equal(flat[off:off + sd[k].numel()], sd[k].reshape(-1)), k          # the offsets of train.param_layout
        assert back[k].data_ptr() == flat.data_ptr() + 4 * off                           # views, nothing copied
        pos += sd[k].numel()
    assert pos == flat.numel()
    assert torch.equal(flatten_state_dict({k: v.numpy() for k, v in sd.items()}, cfg), flat)      # arrays as well as tensors


def test_flatten_refuses_missing_keys_and_wrong_shapes():
    cfg = CONFIGS["d192_64tok"]
    sd = _sd(cfg, 0)
    with pytest.raises(KeyError):
        flatten_state_dict({k: v for k, v in sd.items() if k != "norm.bias"}, cfg)
    with pytest.raises(ValueError):
        flatten_state_dict(dict(sd, **{"norm.bias": sd["norm.bias"][:-1]}), cfg)
    with pytest.raises(ValueError):
        unflatten(torch.zeros(weights.param_count(cfg) + 1), cfg)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_load_flat_without_an_engine_goes_into_the_host_state(name):
    cfg = CONFIGS[name]
    den = Denoiser(**asdict(cfg))                                                       # holds seed-0 weights
    before = den.state_dict()
    sd = _sd(cfg, 1)
    assert den.load_flat(flatten_state_dict(sd, cfg)) is den
    got = den.state_dict()
    assert list(got) == list(before)
    for k in got:
        assert torch.equal(got[k], before[k] if k in BUFFERS else sd[k]), k            # angular_speeds is untouched
        assert got[k].dtype == before[k].dtype and got[k].shape == before[k].shape
    assert den.param_count == weights.param_count(cfg) == sum(p.numel() for p in den.parameters())
    for p, k in zip(den.parameters(), train.param_layout(cfg)):
        assert torch.equal(p, sd[k]), k


def test_load_flat_refuses_wrong_length_dtype_and_rank():
    cfg = CONFIGS["d192_64tok"]
    den = Denoiser(**asdict(cfg))
    before = den.state_dict()
    flat = flatten_state_dict(_sd(cfg, 1), cfg)
    for bad, err in ((flat[:-1], ValueError), (torch.cat([flat, flat[:1]]), ValueError), (flat.double(), TypeError), (flat.to(torch.bfloat16), TypeError),
                     (flat.view(1, -1), ValueError), (flat.numpy(), TypeError)):
        with pytest.raises(err):
            den.load_flat(bad)
    after = den.state_dict()
    assert all(torch.equal(after[k], before[k]) for k in before)                        # a refusal changes nothing


def test_load_state_dict_after_load_flat_wins():
    cfg = CONFIGS["d192_64tok"]
    den = Denoiser(**asdict(cfg))
    a, b = _sd(cfg, 0), _sd(cfg, 1)
    den.load_flat(flatten_state_dict(b, cfg))
    den.load_state_dict(a)
    got = den.state_dict()
    assert all(torch.equal(got[k], a[k]) for k in a)


def test_the_new_entries_are_part_of_the_abi():
    for name in ("tld_engine_param_count", "tld_engine_refresh_weights", "tld_debug_quant_mx8_f32"):
        assert name in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), name), name
    L = _lib.lib()
    assert L.tld_engine_param_count(None) == 0
    assert L.tld_engine_refresh_weights(None, None, 0, None) == 1 and L.tld_last_error()            # TLD_ERR_INVALID, before any HIP call
    assert L.tld_debug_quant_mx8_f32(None, None, None, 4, 128, None) == 1


def test_integer_roundings_equal_the_host_roundings(tmp_path):
    """csrc/tld_refresh_math.h (what the refresh kernels round with) against f32_to_bf16_rne and e4m3_rne on every 251st fp32 bit pattern -- 17 M values
    over every exponent, both signs, NaNs and subnormals (tests/host/refresh_math_main.cpp; stride 1 runs all 2^32)."""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    exe = str(tmp_path / "refresh_math_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(repo, "transformer_latent_diffusion_amd", "csrc"),
                    os.path.join(repo, "tests", "host", "refresh_math_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, "251"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout

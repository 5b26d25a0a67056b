"""The ONE contract of the stage hook (StageStore, csrc/tld_host.h; the block in include/tld_hip.h), asserted through the C ABI on each of the six
handles at its smallest test configuration: shapes and status codes only."""
import ctypes as C
import warnings
from dataclasses import asdict

import numpy as np
import pytest
import torch

from conftest import cfg_from_arr, load_golden, synth_weights
from test_gpu_parity import _dev
from transformer_latent_diffusion_amd import _lib

TLD_ERR_KEY, TLD_ERR_SHAPE = 2, 3
F32P = C.POINTER(C.c_float)


class Handle:
    """call(batch) runs the engine once; stage / shape(batch) name a listed stage and its logical shape; read(name, buf, numel, shape4) -> status"""

    def __init__(self, set_debug, call, read, stage, shape, close=lambda: None):
        self.set_debug, self.call, self.read, self.stage, self.shape, self.close = set_debug, call, read, stage, shape, close


def _denoiser():
    from transformer_latent_diffusion_amd import Denoiser
    g = load_golden("g3_tiny16_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_weights(cfg, g["weight_seed"], g["weight_checksum"]).items()})
    m.reserve(2)
    L, dev = _lib.lib(), _dev()
    t = lambda a, B: torch.from_numpy(np.ascontiguousarray(a[:B])).to(dev)

    def read(name, buf, numel, shape4):
        if shape4 is not None:
            L.tld_engine_stage_shape(m._engine, name, shape4)
        return L.tld_engine_read_stage(m._engine, name, buf, numel)
    ntok = (cfg.image_size // cfg.patch_size) ** 2
    return Handle(m.set_debug, lambda B: m(t(g["x"], B), t(g["sigma"], B), t(g["label"], B)), read, b"blk1.ca", lambda B: [B * ntok, cfg.embed_dim, 1, 1])


def _vae(encoder):
    from transformer_latent_diffusion_amd.vae import AutoencoderKLDecoder, VaeDecoderConfig
    from transformer_latent_diffusion_amd.vae_encoder import AutoencoderKLEncoder, VaeEncoderConfig
    warnings.simplefilter("ignore", RuntimeWarning)            # (the synthetic-weights notice)
    kw = dict(block_out_channels=(64, 128), layers_per_block=1)
    gen = torch.Generator().manual_seed(5)
    if encoder:
        eng = AutoencoderKLEncoder(VaeEncoderConfig(**kw), init_seed=4, max_batch=2)
        x = (torch.randn(2, 3, 64, 64, generator=gen) * 0.6).clamp(-1, 1).to(_dev())
        call, side = (lambda B: eng.moments(x[:B])), 64
    else:
        eng = AutoencoderKLDecoder(VaeDecoderConfig(**kw), init_seed=4, max_batch=2)
        z = torch.randn(2, 4, 8, 8, generator=gen).to(_dev())
        call, side = (lambda B: eng.decode(z[:B])[0]), 8
    call(2)                                                     # builds the engine (debug off)
    return Handle(eng.set_debug, call, lambda name, buf, numel, shape4: eng._abi("read_stage")(eng._engine, name, buf, numel, shape4), b"conv_in",
                  lambda B: [B, 128 if not encoder else 64, side, side], eng._drop_engine)


def _clip():
    from test_clip_host import TINY, _tokens
    from transformer_latent_diffusion_amd.clip_text import ClipTextEncoder, synth_clip_state_dict
    enc = ClipTextEncoder(TINY, max_batch=2)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_clip_state_dict(TINY, 6).items()})
    enc.to(_dev())
    enc._ensure_engine(_dev())
    tok = _tokens(TINY, 2, 3).to(_dev())
    return Handle(enc.set_debug, lambda B: enc.encode_text(tok[:B]), lambda name, buf, numel, shape4: _lib.lib().tld_clip_read_stage(enc._engine, name, buf, numel, shape4),
                  b"blk1.qkv", lambda B: [B * TINY.context_length, 3 * TINY.width, 1, 1], enc._drop_engine)


def _clip_vis():
    from test_clip_vision_host import vcfg
    from transformer_latent_diffusion_amd.clip_image import ClipImageEncoder, synth_clip_visual_state_dict
    cfg = vcfg(14, 2, 64)                                        # 5 tokens, width 64, two layers
    enc = ClipImageEncoder(cfg, max_batch=2)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_clip_visual_state_dict(cfg, 6).items()})
    enc.to(_dev())
    enc._ensure_engine(_dev())
    pix = torch.randn(2, 3, 28, 28, generator=torch.Generator().manual_seed(9)).to(_dev())
    return Handle(enc.set_debug, lambda B: enc.encode_image(pix[:B]), lambda name, buf, numel, shape4: _lib.lib().tld_clip_vis_read_stage(enc._engine, name, buf, numel, shape4),
                  b"blk1.qkv", lambda B: [B * 5, 192, 1, 1], enc._drop_engine)


def _training():
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    cfg = DenoiserConfig(image_size=8, n_channels=4, n_layers=1)          # G = 4, 16 tokens: the smallest grid of tests/test_gpu_train_grids.py
    tr = Trainer(cfg, device=_dev(), init_seed=1, max_batch=2)
    gen = torch.Generator().manual_seed(8)
    x, y, nl = torch.randn(2, 4, 8, 8, generator=gen), torch.randn(2, 768, generator=gen) * 0.5, torch.rand(2, generator=gen) * 0.9 + 0.05
    return Handle(tr.set_debug, lambda B: tr.forward_backward(x[:B] * 0.5, nl[:B], y[:B], x[:B]),
                  lambda name, buf, numel, shape4: _lib.lib().tld_train_read_stage(tr._h, name, buf, numel, shape4), b"blk0.dqkv",
                  lambda B: [B * 16, 3 * cfg.embed_dim, 1, 1])


HANDLES = {"denoiser": _denoiser, "vae_decoder": lambda: _vae(False), "vae_encoder": lambda: _vae(True), "clip": _clip, "clip_vis": _clip_vis, "training": _training}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(HANDLES))
def test_one_stage_hook_contract(which):
    h = HANDLES[which]()
    name = h.stage
    n2 = int(np.prod(h.shape(2)))
    buf = np.full(n2 + 1, -7.0, np.float32)
    ptr, shape = buf.ctypes.data_as(F32P), (C.c_int64 * 4)()
    assert h.read(name, ptr, n2, None) == TLD_ERR_KEY                                   # no debug call yet
    h.set_debug(True)
    h.set_debug(True)                                                                   # twice is harmless
    assert h.read(name, ptr, n2, None) == TLD_ERR_KEY and b"no captured stage named" in _lib.lib().tld_last_error()
    h.call(2)
    assert h.read(name, ptr, n2 - 1, shape) == TLD_ERR_SHAPE and list(shape) == h.shape(2)
    assert (buf == -7.0).all()                                                          # a refused read writes nothing
    assert h.read(name, ptr, n2, shape) == 0 and list(shape) == h.shape(2)
    assert np.isfinite(buf[:n2]).all() and buf[n2] == -7.0
    h.call(1)
    n1 = int(np.prod(h.shape(1)))
    assert h.read(name, ptr, n2, shape) == TLD_ERR_SHAPE and list(shape) == h.shape(1)  # the stage holds the last call
    assert h.read(name, ptr, n1, shape) == 0 and list(shape) == h.shape(1)
    h.set_debug(False)
    assert h.read(name, ptr, n1, None) == TLD_ERR_KEY
    h.close()

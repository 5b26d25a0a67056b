"""``AutoencoderKLEncoder`` / ``AutoencoderKL``: the encode half of the reference's VAE, backed by the gfx950 engine.

The reference's data pipeline turns images into training latents on the GPU (tld/data.py, ``encode_image``):

    x = img.to(device).to(torch.float16) * 2 - 1
    encoded = vae.encode(x, return_dict=False)[0].sample()

where ``vae`` is diffusers' ``AutoencoderKL`` ("madebyollin/sdxl-vae-fp16-fix"; diffusers 0.2x, not installed in this image).
``AutoencoderKLEncoder.encode`` is a drop-in for that call; ``AutoencoderKL`` holds an encoder and an ``AutoencoderKLDecoder``
behind one ``load_state_dict`` and is the drop-in for the whole ``vae`` object of tld/data.py and tld/diffusion.py:

    vae = AutoencoderKL()                                    # SDXL-VAE geometry
    vae.load_state_dict(sd)                                  # a full AutoencoderKL state dict (diffusers key names)
    vae = vae.to("cuda")
    z = vae.encode(x, return_dict=False)[0].sample()         # [B, 3, S, S] in [-1, 1] -> [B, 4, S/8, S/8]
    img = vae.decode(z)[0]

Arithmetic runs in ``libtld_hip.so`` (``tld_vae_enc_*`` in include/tld_hip.h): the decoder's implicit-GEMM 3x3 convolutions,
with a stride-2 addressing mode for the downsamplers, fp32 GroupNorm statistics and softmax.  The engine returns the fp32
moments; ``DiagonalGaussianDistribution`` (torch, on their device) restates diffusers' formulas.  There is no CPU path:
``encode`` without a HIP device raises.  A fresh object holds deterministic random weights.
"""
from __future__ import annotations

import json
import os
import warnings
from collections import OrderedDict
from dataclasses import dataclass
from typing import Mapping, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .vae import AutoencoderKLDecoder, VaeDecoderConfig, _IO_DTYPES, _Spec, _VaeEngine, _batch_limit, _canon_key, _config_from_json, _synth_fill

_NO_CPU = "AutoencoderKLEncoder.encode needs a HIP device (tensors on 'cuda'); there is no CPU path"


@dataclass
class VaeEncoderConfig:
    """The AutoencoderKL config fields the encoder depends on (defaults: SDXL VAE, config.json of the model card)."""
    in_channels: int = 3
    latent_channels: int = 4
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    mid_block_add_attention: bool = True
    use_quant_conv: bool = True

    @property
    def downscale(self) -> int:
        return 2 ** (len(self.block_out_channels) - 1)


def vae_encoder_spec(cfg: VaeEncoderConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered {key: shape} of the encode-side entries of ``AutoencoderKL.state_dict()`` (diffusers >= 0.19 names; forward order)."""
    s = _Spec()
    zc, boc = cfg.latent_channels, tuple(cfg.block_out_channels)
    c = boc[0]
    s.conv("encoder.conv_in", cfg.in_channels, c, 3)
    for i, cout in enumerate(boc):
        for j in range(cfg.layers_per_block):
            s.resnet(f"encoder.down_blocks.{i}.resnets.{j}", c if j == 0 else cout, cout)
        c = cout
        if i != len(boc) - 1:
            s.conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c, c, 3)
    s.mid_block("encoder.mid_block", c, cfg.mid_block_add_attention)
    s.norm("encoder.conv_norm_out", c)
    s.conv("encoder.conv_out", c, 2 * zc, 3)
    if cfg.use_quant_conv:
        s.conv("quant_conv", 2 * zc, 2 * zc, 1)
    return OrderedDict(s)


def synth_vae_encoder_state_dict(cfg: VaeEncoderConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random encoder weights (their own Philox stream, identical on every box), filled like ``synth_vae_state_dict``."""
    return _synth_fill(vae_encoder_spec(cfg), seed + 0x5E1C, lambda k: "to_q" in k or "to_k" in k or k.startswith("quant_conv"))


def encoder_max_activation_elems(cfg: VaeEncoderConfig, image_size: int) -> int:
    """Elements per sample of the encoder's largest activation (mirrors enc_max_act_elems in csrc/tld_vae.hip)."""
    boc = list(cfg.block_out_channels)
    h, c = image_size, boc[0]
    mx = h * h * c
    for i, cout in enumerate(boc):
        mx = max(mx, h * h * max(c, cout))
        c = cout
        if i != len(boc) - 1:
            h //= 2
    return max(mx, h * h * c * 3)


def encoder_batch_limit(cfg: VaeEncoderConfig, image_size: int) -> int:
    """Largest per-call batch the encoder engine accepts at this resolution (``_batch_limit``)."""
    return _batch_limit(encoder_max_activation_elems(cfg, image_size))


def read_vae_encoder_config(path: str) -> VaeEncoderConfig:
    """The encoder fields of a diffusers AutoencoderKL ``config.json`` (a file, or a directory holding one)."""
    if os.path.isdir(path):
        path = os.path.join(path, "config.json")
    with open(path) as f:
        return _config_from_json(VaeEncoderConfig, json.load(f), in_channels=3, use_quant_conv=True)


class DiagonalGaussianDistribution:
    """diffusers' ``DiagonalGaussianDistribution`` over the encoder's moments [B, 2 zc, h, w]:

        mean, logvar = moments.chunk(2, dim=1);  logvar = clamp(logvar, -30, 20)
        std = exp(0.5 logvar);  var = exp(logvar)
        sample(generator) = mean + std * randn(mean.shape, generator)     mode() = mean
        kl() = 0.5 * sum(mean^2 + var - 1 - logvar, dim=[1, 2, 3])
    """

    def __init__(self, parameters: torch.Tensor, deterministic: bool = False):
        self.parameters = parameters
        self.mean, self.logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.deterministic = deterministic
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)
        if deterministic:
            self.var = self.std = torch.zeros_like(self.mean)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        # (diffusers' randn_tensor: a generator on another device draws there and the noise moves to the moments' device)
        dev, dt = self.parameters.device, self.parameters.dtype
        gdev = generator.device if generator is not None else dev
        noise = torch.randn(self.mean.shape, generator=generator, device=gdev, dtype=dt).to(dev)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean

    def kl(self, other: Optional["DiagonalGaussianDistribution"] = None) -> torch.Tensor:
        if self.deterministic:
            return torch.zeros(self.mean.shape[0], device=self.mean.device)
        if other is None:
            return 0.5 * torch.sum(self.mean.pow(2) + self.var - 1.0 - self.logvar, dim=[1, 2, 3])
        return 0.5 * torch.sum((self.mean - other.mean).pow(2) / other.var + self.var / other.var - 1.0 - self.logvar + other.logvar,
                               dim=[1, 2, 3])


class AutoencoderKLOutput(tuple):
    """``vae.encode(x)`` result: ``[0]`` / ``.latent_dist`` is the ``DiagonalGaussianDistribution``."""

    @property
    def latent_dist(self) -> DiagonalGaussianDistribution:
        return self[0]


class AutoencoderKLEncoder(_VaeEngine):
    _ABI, _CALL, _CONFIG = "tld_vae_enc", "encode", _lib.TldVaeEncConfig
    _OTHER_KEYS, _NOUN, _HALF = ("decoder.", "post_quant_conv."), "VAE encoder", "encoder"

    def __init__(self, cfg: Optional[VaeEncoderConfig] = None, init_seed: int = 0, max_batch: int = 16):
        cfg = cfg if cfg is not None else VaeEncoderConfig()
        super().__init__(cfg, vae_encoder_spec(cfg), synth_vae_encoder_state_dict(cfg, init_seed), max_batch)

    def _fill_config(self, cc, size: int):
        cc.in_channels, cc.use_quant_conv, cc.image_size = self.config.in_channels, int(self.config.use_quant_conv), size

    def _ensure_engine(self, device: torch.device, image_size: int):
        # One activation buffer must stay below 4 GiB (32-bit DMA offsets): at large resolutions the engine encodes fewer images
        # per call than max_batch asks for.
        self._ensure_sized_engine(device, image_size, encoder_batch_limit(self.config, image_size))

    @torch.no_grad()
    def moments(self, x: torch.Tensor) -> torch.Tensor:
        """The encoder + quant_conv output: ``[B, in_channels, S, S]`` -> fp32 ``[B, 2 latent_channels, S/8, S/8]`` (mean | logvar)."""
        c = self.config
        if x.dim() != 4 or x.shape[1] != c.in_channels or x.shape[2] != x.shape[3]:
            raise ValueError(f"expected images [B, {c.in_channels}, S, S], got {tuple(x.shape)}")
        if x.dtype not in _IO_DTYPES:
            raise TypeError(f"unsupported image dtype {x.dtype}")
        if x.device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        B, _, S, _ = x.shape
        if S % 64 or S % (8 * c.downscale):
            raise ValueError(f"image size {S}: must be a multiple of 64 and of {8 * c.downscale}")
        if not self._weights_loaded:
            self._weights_loaded = True             # (warn once per object)
            warnings.warn("AutoencoderKLEncoder is encoding with its deterministic RANDOM initialisation: no checkpoint was loaded "
                          "(load_state_dict); the latents are meaningless", RuntimeWarning, stacklevel=3)
        dev = x.device
        x = x.contiguous()
        self._ensure_engine(dev, S)
        s = S // c.downscale
        out = torch.empty(B, 2 * c.latent_channels, s, s, dtype=torch.float32, device=dev)
        self._run(x, out)
        return out

    def encode(self, x: torch.Tensor, return_dict: bool = True, **_ignored) -> Union[AutoencoderKLOutput, Tuple[DiagonalGaussianDistribution]]:
        """``AutoencoderKL.encode(x)``: ``.latent_dist`` (``return_dict=True``) or ``(latent_dist,)`` -- the reference's call."""
        dist = DiagonalGaussianDistribution(self.moments(x))
        return AutoencoderKLOutput((dist,)) if return_dict else (dist,)


class AutoencoderKL:
    """Encoder + decoder behind one object: the ``vae`` of tld/data.py (``.encode(x)[0].sample()``) and tld/diffusion.py
    (``.decode(z)[0]``).  ``load_state_dict`` takes a full AutoencoderKL state dict and routes each key to its half."""

    def __init__(self, encoder_config: Optional[VaeEncoderConfig] = None, decoder_config: Optional[VaeDecoderConfig] = None,
                 init_seed: int = 0, max_batch: int = 16):
        self.encoder = AutoencoderKLEncoder(encoder_config, init_seed=init_seed, max_batch=max_batch)
        self.decoder = AutoencoderKLDecoder(decoder_config, init_seed=init_seed, max_batch=max_batch)

    def eval(self) -> "AutoencoderKL":
        return self

    def to(self, *args, **kwargs) -> "AutoencoderKL":
        self.encoder.to(*args, **kwargs)
        self.decoder.to(*args, **kwargs)
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        sd = self.encoder.state_dict()
        sd.update(self.decoder.state_dict())
        return sd

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], strict: bool = True):
        enc, dec = OrderedDict(), OrderedDict()
        for k, v in sd.items():
            ck = _canon_key(str(k))
            if ck.startswith(("encoder.", "quant_conv.")):
                enc[ck] = v
            elif ck.startswith(("decoder.", "post_quant_conv.")):
                dec[ck] = v
            elif strict:
                raise RuntimeError(f"unexpected key {k!r} in AutoencoderKL state_dict")
        self.encoder.load_state_dict(enc, strict=strict)
        self.decoder.load_state_dict(dec, strict=strict)
        return self

    def parameters(self):
        yield from self.encoder.parameters()
        yield from self.decoder.parameters()

    def encode(self, x: torch.Tensor, return_dict: bool = True, **kw):
        return self.encoder.encode(x, return_dict=return_dict, **kw)

    def decode(self, z: torch.Tensor, return_dict: bool = False, **kw):
        return self.decoder.decode(z, return_dict=return_dict, **kw)


@torch.no_grad()
def encode_image(img: torch.Tensor, vae, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """tld/data.py ``encode_image``: pixels in [0, 1] -> ``vae.encode(img * 2 - 1)[0].sample()`` (the reference casts to fp16 first)."""
    x = img.to(torch.float16) * 2 - 1
    return vae.encode(x, return_dict=False)[0].sample(generator=generator)

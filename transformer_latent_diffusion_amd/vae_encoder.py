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

import ctypes as C
import json
import os
import warnings
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Mapping, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from .vae import AutoencoderKLDecoder, VaeDecoderConfig, _canon_key

_IO_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}
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
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    zc, boc = cfg.latent_channels, tuple(cfg.block_out_channels)

    def conv(prefix, cin, cout, k):
        s[prefix + ".weight"] = (cout, cin, k, k)
        s[prefix + ".bias"] = (cout,)

    def norm(prefix, c):
        s[prefix + ".weight"] = (c,)
        s[prefix + ".bias"] = (c,)

    def resnet(prefix, cin, cout):
        norm(prefix + ".norm1", cin)
        conv(prefix + ".conv1", cin, cout, 3)
        norm(prefix + ".norm2", cout)
        conv(prefix + ".conv2", cout, cout, 3)
        if cin != cout:
            conv(prefix + ".conv_shortcut", cin, cout, 1)

    conv("encoder.conv_in", cfg.in_channels, boc[0], 3)
    c = boc[0]
    for i, cout in enumerate(boc):
        for j in range(cfg.layers_per_block):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", c if j == 0 else cout, cout)
        c = cout
        if i != len(boc) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", c, c, 3)
    resnet("encoder.mid_block.resnets.0", c, c)
    if cfg.mid_block_add_attention:
        a = "encoder.mid_block.attentions.0"
        norm(a + ".group_norm", c)
        for n in ("to_q", "to_k", "to_v", "to_out.0"):
            s[f"{a}.{n}.weight"] = (c, c)
            s[f"{a}.{n}.bias"] = (c,)
    resnet("encoder.mid_block.resnets.1", c, c)
    norm("encoder.conv_norm_out", c)
    conv("encoder.conv_out", c, 2 * zc, 3)
    if cfg.use_quant_conv:
        conv("quant_conv", 2 * zc, 2 * zc, 1)
    return s


def synth_vae_encoder_state_dict(cfg: VaeEncoderConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random encoder weights (their own Philox stream, identical on every box), filled like ``synth_vae_state_dict``:
    variance-preserving conv / linear gains, GroupNorm affines away from identity, non-zero biases."""
    rng = np.random.Generator(np.random.Philox(key=seed + 0x5E1C))
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in vae_encoder_spec(cfg).items():
        if ".norm" in k or "group_norm" in k or "conv_norm_out" in k:
            v = (1.0 + 0.2 * rng.standard_normal(shape)) if k.endswith(".weight") else 0.1 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            gain = 1.0 if ("to_q" in k or "to_k" in k or k.startswith("quant_conv")) else 1.3
            v = gain * rng.standard_normal(shape) / np.sqrt(fan_in)
        out[k] = np.asarray(v, dtype=np.float32)
    return out


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
    """Largest per-call batch the encoder engine accepts at this resolution: one bf16 activation buffer (+ its 2-KiB zero page) < 4 GiB."""
    return int(((1 << 32) - 2048 - 1) // (2 * encoder_max_activation_elems(cfg, image_size)))


def read_vae_encoder_config(path: str) -> VaeEncoderConfig:
    """The encoder fields of a diffusers AutoencoderKL ``config.json`` (a file, or a directory holding one)."""
    if os.path.isdir(path):
        path = os.path.join(path, "config.json")
    with open(path) as f:
        j = json.load(f)
    return VaeEncoderConfig(in_channels=j.get("in_channels", 3), latent_channels=j.get("latent_channels", 4),
                            block_out_channels=tuple(j.get("block_out_channels", (64,))), layers_per_block=j.get("layers_per_block", 1),
                            norm_num_groups=j.get("norm_num_groups", 32), mid_block_add_attention=j.get("mid_block_add_attention", True),
                            use_quant_conv=j.get("use_quant_conv", True))


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


class AutoencoderKLEncoder:
    def __init__(self, cfg: Optional[VaeEncoderConfig] = None, init_seed: int = 0, max_batch: int = 16):
        self.config = cfg if cfg is not None else VaeEncoderConfig()
        self._spec = vae_encoder_spec(self.config)
        self._state: "OrderedDict[str, torch.Tensor]" = OrderedDict(
            (k, torch.from_numpy(v)) for k, v in synth_vae_encoder_state_dict(self.config, init_seed).items())
        self._weights_loaded = False     # still on the deterministic random initialisation
        self.max_batch = int(max_batch)          # images per engine call; larger batches are encoded in chunks
        self._device: Optional[torch.device] = None
        self._engine = None
        self._engine_key = None

    # ---- nn.Module-like surface ----------------------------------------------------------------------------------
    def eval(self) -> "AutoencoderKLEncoder":
        return self

    def to(self, *args, **kwargs) -> "AutoencoderKLEncoder":
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.dtype):
                continue                          # moments are fp32; the engine computes in bf16 / fp32 regardless
            if isinstance(a, (torch.device, str)):
                dev = torch.device(a)
                if dev != self._device:
                    self._drop_engine()
                self._device = dev
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict(self._state)

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], strict: bool = True):
        new = OrderedDict()
        seen = set()
        for k, v in sd.items():
            k = _canon_key(str(k))
            if k.startswith("decoder.") or k.startswith("post_quant_conv."):
                continue
            if k not in self._spec:
                if strict:
                    raise RuntimeError(f"unexpected key {k!r} in VAE encoder state_dict")
                continue
            t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().cpu().to(torch.float32)
            want = self._spec[k]
            if tuple(t.shape) != tuple(want):
                if t.numel() == int(np.prod(want)) and tuple(s for s in t.shape if s != 1) == tuple(s for s in want if s != 1):
                    t = t.reshape(want)           # Linear [C, C] vs 1x1-conv [C, C, 1, 1] spellings of the attention block
                else:
                    raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(t.shape)}, model {tuple(want)}")
            new[k] = t.contiguous()
            seen.add(k)
        missing = [k for k in self._spec if k not in seen]
        if strict and missing:
            raise RuntimeError(f"missing keys in VAE encoder state_dict: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self._state.update(new)
        self._weights_loaded = True
        self._drop_engine()
        return self

    def parameters(self):
        return iter(self._state.values())

    # ---- engine ---------------------------------------------------------------------------------------------------
    def _drop_engine(self):
        if self._engine is not None:
            _lib.lib().tld_vae_enc_destroy(self._engine)
            self._engine = None
            self._engine_key = None

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _ensure_engine(self, device: torch.device, image_size: int):
        # (sized once per resolution.)  One activation buffer must stay below 4 GiB (32-bit DMA offsets): at large resolutions
        # the engine encodes fewer images per call than max_batch asks for.
        nb = max(1, min(self.max_batch, encoder_batch_limit(self.config, image_size)))
        key = (device.index or 0, image_size, nb)
        if self._engine is not None and self._engine_key == key:
            return
        self._drop_engine()
        L = _lib.lib()
        c = self.config
        if len(c.block_out_channels) > 4:
            raise RuntimeError("at most 4 encoder blocks are supported")
        cc = _lib.TldVaeEncConfig()
        cc.in_channels, cc.latent_channels, cc.n_blocks = c.in_channels, c.latent_channels, len(c.block_out_channels)
        for i, v in enumerate(c.block_out_channels):
            cc.block_out_channels[i] = int(v)
        cc.layers_per_block, cc.norm_num_groups = c.layers_per_block, c.norm_num_groups
        cc.mid_block_attention, cc.use_quant_conv = int(c.mid_block_add_attention), int(c.use_quant_conv)
        cc.image_size, cc.max_batch, cc.device_id = image_size, nb, device.index or 0
        h = C.c_void_p()
        _lib.check(L.tld_vae_enc_create(C.byref(cc), C.byref(h)), "tld_vae_enc_create")
        try:
            for k, t in self._state.items():
                a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(L.tld_vae_enc_load_tensor(h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, _lib.DTYPE_F32),
                           f"tld_vae_enc_load_tensor({k})")
            _lib.check(L.tld_vae_enc_finalize_weights(h), "tld_vae_enc_finalize_weights")
        except Exception:
            L.tld_vae_enc_destroy(h)
            raise
        self._engine, self._engine_key = h, key

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
        L = _lib.lib()
        s = S // c.downscale
        out = torch.empty(B, 2 * c.latent_channels, s, s, dtype=torch.float32, device=dev)
        nb = self._engine_key[2]
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for b0 in range(0, B, nb):
                b1 = min(B, b0 + nb)
                _lib.check(L.tld_vae_enc_encode(self._engine, C.c_void_p(x[b0:b1].data_ptr()), C.c_void_p(out[b0:b1].data_ptr()),
                                                b1 - b0, _IO_DTYPES[x.dtype], C.c_void_p(stream)), "tld_vae_enc_encode")
        return out

    def encode(self, x: torch.Tensor, return_dict: bool = True, **_ignored) -> Union[AutoencoderKLOutput, Tuple[DiagonalGaussianDistribution]]:
        """``AutoencoderKL.encode(x)``: ``.latent_dist`` (``return_dict=True``) or ``(latent_dist,)`` -- the reference's call."""
        dist = DiagonalGaussianDistribution(self.moments(x))
        return AutoencoderKLOutput((dist,)) if return_dict else (dist,)

    # ---- test / profiling hooks -----------------------------------------------------------------------------------
    def set_debug(self, on: bool = True):
        _lib.check(_lib.lib().tld_vae_enc_set_debug(self._engine, int(on)), "tld_vae_enc_set_debug")

    def read_stage(self, name: str) -> torch.Tensor:
        L = _lib.lib()
        shape = (C.c_int64 * 4)()
        probe = np.empty(1, dtype=np.float32)
        L.tld_vae_enc_read_stage(self._engine, name.encode(), probe.ctypes.data_as(C.POINTER(C.c_float)), -1, shape)
        if shape[0] == 0:
            _lib.check(1, f"tld_vae_enc_read_stage({name})")
        out = np.empty(tuple(shape), dtype=np.float32)
        _lib.check(L.tld_vae_enc_read_stage(self._engine, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, shape),
                   f"tld_vae_enc_read_stage({name})")
        return torch.from_numpy(out)

    def set_profile(self, on: bool = True):
        _lib.check(_lib.lib().tld_vae_enc_set_profile(self._engine, int(on)), "tld_vae_enc_set_profile")

    def get_profile(self) -> Dict[str, Tuple[float, int]]:
        L = _lib.lib()
        res = {}
        for i, name in enumerate(_lib.VAE_KERNEL_CLASSES):
            ms, n = C.c_double(), C.c_int64()
            _lib.check(L.tld_vae_enc_get_profile(self._engine, i, C.byref(ms), C.byref(n)), "tld_vae_enc_get_profile")
            res[name] = (ms.value, n.value)
        return res

    @property
    def weight_bytes(self) -> int:
        return int(_lib.lib().tld_vae_enc_weight_bytes(self._engine)) if self._engine is not None else 0


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

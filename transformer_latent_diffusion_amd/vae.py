"""``AutoencoderKLDecoder``: the decode half of the reference's VAE, backed by the gfx950 engine.

The reference's sampler ends with ``self.vae.decode((x0_pred * scale_factor).to(dtype))[0].cpu()``
(tld/diffusion.py:91), where ``vae`` is ``diffusers.AutoencoderKL.from_pretrained("madebyollin/sdxl-vae-fp16-fix")``
(tld/diffusion.py:146, tld/configs.py:39-43) -- a third-party model (diffusers 0.2x; not part of the reference checkout,
not installed in this image).  This class is a drop-in for that one call:

    vae = AutoencoderKLDecoder(VaeDecoderConfig())          # SDXL-VAE geometry: (128, 256, 512, 512), 2 layers per block
    vae.load_state_dict(sd)                                  # AutoencoderKL key names; encoder / quant_conv entries ignored
    vae = vae.to("cuda")
    img = vae.decode(latents)[0]                             # [B, 4, h, w] -> [B, 3, 8h, 8w] fp32, same device

and is what ``DiffusionGenerator(model, vae, device, dtype)`` takes as ``vae``.  Arithmetic runs in ``libtld_hip.so``
(``tld_vae_*`` in include/tld_hip.h: implicit-GEMM 3x3 convolutions on bf16 MFMA, fp32 GroupNorm statistics and
softmax); there is no CPU path -- ``decode`` without a HIP device raises.  A fresh object holds deterministic random
weights (like ``nn.Module`` construction; no checkpoint can be downloaded here).
"""
from __future__ import annotations

import ctypes as C
import warnings
import json
import os
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib

_IO_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


@dataclass
class VaeDecoderConfig:
    """The AutoencoderKL config fields the decoder depends on (defaults: SDXL VAE, config.json of the model card)."""
    latent_channels: int = 4
    out_channels: int = 3
    block_out_channels: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    mid_block_add_attention: bool = True
    use_post_quant_conv: bool = True

    @property
    def upscale(self) -> int:
        return 2 ** (len(self.block_out_channels) - 1)


class _Spec(OrderedDict):
    """Ordered {key: shape} under construction: the layer kinds both halves of ``AutoencoderKL.state_dict()`` are made of."""

    def conv(self, prefix, cin, cout, k):
        self[prefix + ".weight"] = (cout, cin, k, k)
        self[prefix + ".bias"] = (cout,)

    def norm(self, prefix, c):
        self[prefix + ".weight"] = (c,)
        self[prefix + ".bias"] = (c,)

    def resnet(self, prefix, cin, cout):
        self.norm(prefix + ".norm1", cin)
        self.conv(prefix + ".conv1", cin, cout, 3)
        self.norm(prefix + ".norm2", cout)
        self.conv(prefix + ".conv2", cout, cout, 3)
        if cin != cout:
            self.conv(prefix + ".conv_shortcut", cin, cout, 1)

    def mid_block(self, prefix, c, attention):
        self.resnet(prefix + ".resnets.0", c, c)
        if attention:
            a = prefix + ".attentions.0"
            self.norm(a + ".group_norm", c)
            for n in ("to_q", "to_k", "to_v", "to_out.0"):
                self[f"{a}.{n}.weight"] = (c, c)
                self[f"{a}.{n}.bias"] = (c,)
        self.resnet(prefix + ".resnets.1", c, c)


def vae_decoder_spec(cfg: VaeDecoderConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered {key: shape} of the decode-side entries of ``AutoencoderKL.state_dict()`` (diffusers >= 0.19 names)."""
    s = _Spec()
    zc, boc = cfg.latent_channels, tuple(cfg.block_out_channels)
    c = boc[-1]
    if cfg.use_post_quant_conv:
        s.conv("post_quant_conv", zc, zc, 1)
    s.conv("decoder.conv_in", zc, c, 3)
    s.mid_block("decoder.mid_block", c, cfg.mid_block_add_attention)
    for i, cout in enumerate(reversed(boc)):
        for j in range(cfg.layers_per_block + 1):
            s.resnet(f"decoder.up_blocks.{i}.resnets.{j}", c if j == 0 else cout, cout)
        c = cout
        if i != len(boc) - 1:
            s.conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", c, c, 3)
    s.norm("decoder.conv_norm_out", c)
    s.conv("decoder.conv_out", c, cfg.out_channels, 3)
    return OrderedDict(s)


def _synth_fill(spec: Mapping[str, Tuple[int, ...]], key: int, unit_gain) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random weights for ``spec``, drawn in its order from the Philox stream ``key`` (identical on every box):
    variance-preserving conv / linear gains (1.0 where ``unit_gain(name)``, else 1.3: SiLU halves variance), GroupNorm affines away
    from identity, non-zero biases."""
    rng = np.random.Generator(np.random.Philox(key=key))
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in spec.items():
        if ".norm" in k or "group_norm" in k or "conv_norm_out" in k:
            v = (1.0 + 0.2 * rng.standard_normal(shape)) if k.endswith(".weight") else 0.1 * rng.standard_normal(shape)
        elif k.endswith(".bias"):
            v = 0.05 * rng.standard_normal(shape)
        else:
            fan_in = int(np.prod(shape[1:]))
            v = (1.0 if unit_gain(k) else 1.3) * rng.standard_normal(shape) / np.sqrt(fan_in)
        out[k] = np.asarray(v, dtype=np.float32)
    return out


def synth_vae_state_dict(cfg: VaeDecoderConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random decoder weights (``_synth_fill``; attention logits with O(1) spread) -- a numerically interesting
    stand-in for the checkpoint that cannot be downloaded here."""
    return _synth_fill(vae_decoder_spec(cfg), seed + 0x5D1, lambda k: "to_q" in k or "to_k" in k)


def max_activation_elems(cfg: VaeDecoderConfig, latent_size: int) -> int:
    """Elements per sample of the decoder's largest activation (what sizes the engine's four ping-pong buffers; mirrors
    max_act_elems in csrc/tld_vae.hip)."""
    boc = list(cfg.block_out_channels)
    h, c = latent_size, boc[-1]
    mx = h * h * c * 3                                   # attention q | k | v
    for i, cout in enumerate(reversed(boc)):
        mx = max(mx, h * h * max(c, cout))
        c = cout
        if i != len(boc) - 1:
            h *= 2
            mx = max(mx, h * h * c)
    return mx


def _batch_limit(elems_per_sample: int) -> int:
    """Largest per-call batch an engine accepts: one bf16 activation buffer (+ its 2-KiB zero page) must stay below 4 GiB."""
    return int(((1 << 32) - 2048 - 1) // (2 * elems_per_sample))


def engine_batch_limit(cfg: VaeDecoderConfig, latent_size: int) -> int:
    """Largest per-call batch the decoder engine accepts at this resolution (``_batch_limit``)."""
    return _batch_limit(max_activation_elems(cfg, latent_size))


_OLD_ATTN = ((".query.", ".to_q."), (".key.", ".to_k."), (".value.", ".to_v."), (".proj_attn.", ".to_out.0."))


def _canon_key(k: str) -> str:
    if ".attentions." in k:
        for old, new in _OLD_ATTN:
            k = k.replace(old, new)
    return k


def _config_from_json(cls, j: Mapping, **own):
    """``cls`` from the dict of a diffusers AutoencoderKL ``config.json``: the fields both halves share + ``own`` {field: default}."""
    return cls(latent_channels=j.get("latent_channels", 4), block_out_channels=tuple(j.get("block_out_channels", (64,))),
               layers_per_block=j.get("layers_per_block", 1), norm_num_groups=j.get("norm_num_groups", 32),
               mid_block_add_attention=j.get("mid_block_add_attention", True), **{k: j.get(k, d) for k, d in own.items()})


def load_vae_checkpoint(path: str) -> Tuple["OrderedDict[str, torch.Tensor]", Optional[VaeDecoderConfig]]:
    """Read a diffusers AutoencoderKL checkpoint: a directory (``config.json`` + ``diffusion_pytorch_model.safetensors``
    or ``.bin``) or a single weights file.  Returns (state_dict, config or None)."""
    cfg = None
    wfile = path
    if os.path.isdir(path):
        cj = os.path.join(path, "config.json")
        if os.path.exists(cj):
            with open(cj) as f:
                cfg = _config_from_json(VaeDecoderConfig, json.load(f), out_channels=3, use_post_quant_conv=True)
        for name in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin"):
            if os.path.exists(os.path.join(path, name)):
                wfile = os.path.join(path, name)
                break
        else:
            raise FileNotFoundError(f"{path}: no diffusion_pytorch_model.safetensors / .bin")
    if wfile.endswith(".safetensors"):
        from safetensors.torch import load_file
        sd = load_file(wfile)
    else:
        sd = torch.load(wfile, map_location="cpu", weights_only=True)
    return OrderedDict((_canon_key(k), v) for k, v in sd.items()), cfg


class DecoderOutput(tuple):
    """``vae.decode(z)`` result: indexable like diffusers' (``[0]`` is the image batch) with a ``.sample`` attribute."""

    @property
    def sample(self) -> torch.Tensor:
        return self[0]


class _VaeEngine:
    """What ``AutoencoderKLDecoder`` and ``AutoencoderKLEncoder`` share: the nn.Module-like surface over a host state dict, the
    lifecycle of one native engine (create / load / finalize, destroyed on an error and when weights or device change), the chunked
    call and the test hooks.  A subclass names its half of the C ABI and of the state dict in the class attributes below, fills the
    fields of the config struct that only it has (``_fill_config``) and keeps its shape checks and its public call."""
    _ABI = ""                 # prefix of the C-ABI entries: "tld_vae" / "tld_vae_enc"
    _CALL = ""                # the entry after the prefix that runs a batch: "decode" / "encode"
    _CONFIG = None            # the ctypes config struct of <_ABI>_create
    _OTHER_KEYS = ()          # state-dict prefixes of the other half: passed over by load_state_dict
    _NOUN = ""                # "VAE" / "VAE encoder" in load_state_dict's messages
    _HALF = ""                # "decoder" / "encoder"

    def __init__(self, cfg, spec, state, max_batch: int):
        self.config = cfg
        self._spec = spec
        self._state: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, torch.from_numpy(v)) for k, v in state.items())
        self._weights_loaded = False     # still on the deterministic random initialisation (no checkpoint can be downloaded here)
        self.max_batch = int(max_batch)          # samples per engine call; larger batches go through in chunks
        self._device: Optional[torch.device] = None
        self._engine = None
        self._engine_key = None

    # ---- nn.Module-like surface ----------------------------------------------------------------------------------
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.dtype):
                continue                          # outputs are fp32; the engine computes in bf16 / fp32 regardless
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
            if k.startswith(self._OTHER_KEYS):
                continue
            if k not in self._spec:
                if strict:
                    raise RuntimeError(f"unexpected key {k!r} in {self._NOUN} state_dict")
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
            raise RuntimeError(f"missing keys in {self._NOUN} state_dict: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        self._state.update(new)
        self._weights_loaded = True
        self._drop_engine()
        return self

    def parameters(self):
        return iter(self._state.values())

    # ---- engine ---------------------------------------------------------------------------------------------------
    def _abi(self, entry: str):
        return getattr(_lib.lib(), f"{self._ABI}_{entry}")

    def _check(self, rc: int, entry: str):
        _lib.check(rc, f"{self._ABI}_{entry}")

    def _drop_engine(self):
        if self._engine is not None:
            self._abi("destroy")(self._engine)
            self._engine = None
            self._engine_key = None

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _fill_config(self, cc, size: int):
        raise NotImplementedError

    def _ensure_sized_engine(self, device: torch.device, size: int, limit: int):
        """An engine on ``device`` for inputs of side ``size``, taking min(max_batch, limit) samples per call (sized once per
        resolution: a smaller first batch must not rebuild it later).  ``_engine_key`` is (device index, size, samples per call)."""
        nb = max(1, min(self.max_batch, limit))
        key = (device.index or 0, size, nb)
        if self._engine is not None and self._engine_key == key:
            return
        self._drop_engine()
        c = self.config
        if len(c.block_out_channels) > 4:
            raise RuntimeError(f"at most 4 {self._HALF} blocks are supported")
        cc = self._CONFIG()
        cc.latent_channels, cc.n_blocks = c.latent_channels, len(c.block_out_channels)
        for i, v in enumerate(c.block_out_channels):
            cc.block_out_channels[i] = int(v)
        cc.layers_per_block, cc.norm_num_groups, cc.mid_block_attention = c.layers_per_block, c.norm_num_groups, int(c.mid_block_add_attention)
        cc.max_batch, cc.device_id = nb, device.index or 0
        self._fill_config(cc, size)
        h = C.c_void_p()
        self._check(self._abi("create")(C.byref(cc), C.byref(h)), "create")
        try:
            for k, t in self._state.items():
                a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                self._check(self._abi("load_tensor")(h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, _lib.DTYPE_F32), f"load_tensor({k})")
            self._check(self._abi("finalize_weights")(h), "finalize_weights")
        except Exception:
            self._abi("destroy")(h)
            raise
        self._engine, self._engine_key = h, key

    def _run(self, x: torch.Tensor, out: torch.Tensor):
        """The engine's call over batch ``x`` into ``out`` (both on the engine's device), at most ``_engine_key[2]`` samples at a time."""
        call, nb = self._abi(self._CALL), self._engine_key[2]
        stream = torch.cuda.current_stream(x.device).cuda_stream
        with torch.cuda.device(x.device):
            for b0 in range(0, x.shape[0], nb):
                b1 = min(x.shape[0], b0 + nb)
                self._check(call(self._engine, C.c_void_p(x[b0:b1].data_ptr()), C.c_void_p(out[b0:b1].data_ptr()), b1 - b0, _IO_DTYPES[x.dtype],
                                 C.c_void_p(stream)), self._CALL)

    # ---- test / profiling hooks -----------------------------------------------------------------------------------
    def set_debug(self, on: bool = True):
        self._check(self._abi("set_debug")(self._engine, int(on)), "set_debug")

    def read_stage(self, name: str) -> torch.Tensor:
        read = self._abi("read_stage")
        shape = (C.c_int64 * 4)()
        probe = np.empty(1, dtype=np.float32)
        read(self._engine, name.encode(), probe.ctypes.data_as(C.POINTER(C.c_float)), -1, shape)
        if shape[0] == 0:
            self._check(1, f"read_stage({name})")
        out = np.empty(tuple(shape), dtype=np.float32)
        self._check(read(self._engine, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, shape), f"read_stage({name})")
        return torch.from_numpy(out)

    def set_profile(self, on: bool = True):
        self._check(self._abi("set_profile")(self._engine, int(on)), "set_profile")

    def get_profile(self) -> Dict[str, Tuple[float, int]]:
        res = {}
        for i, name in enumerate(_lib.VAE_KERNEL_CLASSES):
            ms, n = C.c_double(), C.c_int64()
            self._check(self._abi("get_profile")(self._engine, i, C.byref(ms), C.byref(n)), "get_profile")
            res[name] = (ms.value, n.value)
        return res

    @property
    def weight_bytes(self) -> int:
        return int(self._abi("weight_bytes")(self._engine)) if self._engine is not None else 0


class AutoencoderKLDecoder(_VaeEngine):
    _ABI, _CALL, _CONFIG = "tld_vae", "decode", _lib.TldVaeConfig
    _OTHER_KEYS, _NOUN, _HALF = ("encoder.", "quant_conv."), "VAE", "decoder"
    _NO_CPU = "AutoencoderKLDecoder.decode needs a HIP device (tensors on 'cuda'); there is no CPU path"

    def __init__(self, cfg: Optional[VaeDecoderConfig] = None, init_seed: int = 0, max_batch: int = 16):
        cfg = cfg if cfg is not None else VaeDecoderConfig()
        super().__init__(cfg, vae_decoder_spec(cfg), synth_vae_state_dict(cfg, init_seed), max_batch)
        self.dtype = torch.float32               # dtype of the returned images (the reference's vae_dtype)

    def _fill_config(self, cc, size: int):
        cc.out_channels, cc.use_post_quant_conv, cc.latent_size = self.config.out_channels, int(self.config.use_post_quant_conv), size

    def _ensure_engine(self, device: torch.device, latent_size: int, batch: int):
        if device.type != "cuda":
            raise RuntimeError(self._NO_CPU)
        # One activation buffer must stay below 4 GiB (32-bit DMA offsets): at large resolutions the engine decodes fewer samples
        # per call than max_batch asks for.
        self._ensure_sized_engine(device, latent_size, engine_batch_limit(self.config, latent_size))

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = False, **_ignored) -> DecoderOutput:
        """``AutoencoderKL.decode(z)``: ``[B, latent_channels, h, w]`` -> ``([B, out_channels, 8h, 8w] fp32,)``."""
        if z.dim() != 4 or z.shape[1] != self.config.latent_channels or z.shape[2] != z.shape[3]:
            raise ValueError(f"expected latents [B, {self.config.latent_channels}, s, s], got {tuple(z.shape)}")
        if z.dtype not in _IO_DTYPES:
            raise TypeError(f"unsupported latent dtype {z.dtype}")
        dev = z.device if z.device.type == "cuda" else (self._device or z.device)
        if dev.type != "cuda":
            raise RuntimeError(self._NO_CPU)
        if not self._weights_loaded:
            self._weights_loaded = True             # (warn once per object)
            warnings.warn("AutoencoderKLDecoder is decoding with its deterministic RANDOM initialisation: no checkpoint was loaded "
                          "(load_state_dict / load_vae_checkpoint); the images are noise", RuntimeWarning, stacklevel=2)
        z = z.to(dev).contiguous()
        B, _, s, _ = z.shape
        self._ensure_engine(dev, s, B)
        S = s * self.config.upscale
        out = torch.empty(B, self.config.out_channels, S, S, dtype=torch.float32, device=dev)
        self._run(z, out)
        return DecoderOutput((out,))

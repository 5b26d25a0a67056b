"""``ClipTextEncoder``: CLIP's text tower on the gfx950 engine -- the pipeline's front edge.

The reference turns prompts into the denoiser's ``label`` with (tld/diffusion.py:136-140)

    text_tokens = clip.tokenize(label, truncate=True).to(device)
    text_encoding = model.encode_text(text_tokens)

where ``model`` is OpenAI CLIP "ViT-L/14" from ``clip.load`` (tld/diffusion.py:160, tld/configs.py:46-48) -- a third-party
package (openai/CLIP, unpinned in the reference; not in the reference checkout, not installed here).  This class is a
drop-in for the ``model`` of that call: ``ClipTextEncoder(cfg).load_state_dict(clip_state_dict).to("cuda").encode_text(tokens)``
returns ``[B, 768]`` on the tokens' device, so ``DiffusionTransformer(cfg, clip_model=ClipTextEncoder(...))`` keeps the
labels on the GPU.  Tokenisation (BPE over CLIP's merges file) is clip_tokenizer.py's ``ClipTokenizer.tokenize`` or ``clip.tokenize``.

Arithmetic runs in ``libtld_hip.so`` (``tld_clip_*``: bf16 MFMA projections, fp32 residual stream / LayerNorm / softmax);
there is no CPU path.  A fresh object holds deterministic random weights (no checkpoint can be downloaded here).
"""
from __future__ import annotations

import ctypes as C
import warnings
from collections import OrderedDict
from dataclasses import dataclass
from typing import Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib


@dataclass
class ClipTextConfig:
    """Text-side fields of CLIP's constructor (defaults: ViT-L/14)."""
    vocab_size: int = 49408
    context_length: int = 77
    width: int = 768              # transformer_width
    heads: int = 12               # transformer_heads (= width // 64)
    layers: int = 12              # transformer_layers
    embed_dim: int = 768


_METADATA_KEYS = ("logit_scale", "input_resolution", "context_length", "vocab_size")      # the scalars of a CLIP archive: no tower reads them


def _block_spec(s: "OrderedDict[str, Tuple[int, ...]]", prefix: str, layers: int, w: int) -> None:
    """The twelve entries of each ResidualAttentionBlock under ``<prefix><i>.``, in ``state_dict()`` order (both towers)."""
    for i in range(layers):
        p = f"{prefix}{i}."
        s[p + "attn.in_proj_weight"] = (3 * w, w)
        s[p + "attn.in_proj_bias"] = (3 * w,)
        s[p + "attn.out_proj.weight"] = (w, w)
        s[p + "attn.out_proj.bias"] = (w,)
        s[p + "ln_1.weight"] = (w,)
        s[p + "ln_1.bias"] = (w,)
        s[p + "mlp.c_fc.weight"] = (4 * w, w)
        s[p + "mlp.c_fc.bias"] = (4 * w,)
        s[p + "mlp.c_proj.weight"] = (w, 4 * w)
        s[p + "mlp.c_proj.bias"] = (w,)
        s[p + "ln_2.weight"] = (w,)
        s[p + "ln_2.bias"] = (w,)


def _synth_transformer_entry(rng: np.random.Generator, k: str, shape: Tuple[int, ...], w: int, layers: int):
    """One draw for a LayerNorm affine, a bias or a block's matrix (both towers; every other entry is its tower's own)."""
    proj_std, attn_std, fc_std = (w ** -0.5) * ((2 * layers) ** -0.5), w ** -0.5, (2 * w) ** -0.5
    if ".ln_" in k or k.startswith("ln_final"):
        return (1.0 + 0.2 * rng.standard_normal(shape)) if k.endswith("weight") else 0.1 * rng.standard_normal(shape)
    if k.endswith("bias"):
        return 0.05 * rng.standard_normal(shape)
    if "in_proj_weight" in k:
        return 1.5 * attn_std * rng.standard_normal(shape)           # (logits of std ~2 after LayerNorm: a peaked, not degenerate, softmax)
    if "out_proj.weight" in k or "c_proj.weight" in k:
        return 4.0 * proj_std * rng.standard_normal(shape)
    return fc_std * rng.standard_normal(shape)


def clip_text_spec(cfg: ClipTextConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered {key: shape} of the text-side entries of ``CLIP.state_dict()`` (openai/CLIP clip/model.py)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    w = cfg.width
    s["positional_embedding"] = (cfg.context_length, w)
    s["text_projection"] = (w, cfg.embed_dim)
    _block_spec(s, "transformer.resblocks.", cfg.layers, w)
    s["token_embedding.weight"] = (cfg.vocab_size, w)
    s["ln_final.weight"] = (w,)
    s["ln_final.bias"] = (w,)
    return s


def synth_clip_state_dict(cfg: ClipTextConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random text-tower weights (Philox): CLIP's own initialisation scales (clip/model.py initialize_parameters)
    with non-trivial LayerNorm affines and biases, so attention is not uniform and every term of the graph is exercised."""
    rng = np.random.Generator(np.random.Philox(key=seed + 0xC11F))
    w = cfg.width
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in clip_text_spec(cfg).items():
        if k == "token_embedding.weight":
            v = 0.02 * rng.standard_normal(shape, dtype=np.float32)
        elif k == "positional_embedding":
            v = 0.01 * rng.standard_normal(shape)
        elif k == "text_projection":
            v = w ** -0.5 * rng.standard_normal(shape)
        else:
            v = _synth_transformer_entry(rng, k, shape, w, cfg.layers)
        out[k] = np.asarray(v, dtype=np.float32)
    return out


class _ClipEngine:
    """What ``ClipTextEncoder`` and ``ClipImageEncoder`` (clip_image.py) share: the nn.Module-like surface over a host state dict, the lifecycle of
    one native engine (create / load / finalize, destroyed on an error and when weights or device change), the stage hook and the chunked call.
    A subclass names its half of the C ABI and the words of its messages in the class attributes below, fills its config struct (``_config``),
    says which keys of a full CLIP dict are the other tower's (``_is_foreign``) and keeps its argument checks and its public call."""
    _ABI = ""                 # prefix of the C-ABI entries: "tld_clip" / "tld_clip_vis"
    _CALL = ""                # the entry after the prefix that runs a batch, and the public method: "encode_text" / "encode_image"
    _INPUT = ""               # "tokens" / "pixels" in the no-device message

    def __init__(self, cfg, spec, synth, init_seed: int, max_batch: int):
        self.config = cfg
        if cfg.heads * 64 != cfg.width:
            raise ValueError("head_dim must be 64 (width // heads)")
        self._spec = spec(cfg)
        self._state: "OrderedDict[str, torch.Tensor]" = OrderedDict((k, torch.from_numpy(v)) for k, v in synth(cfg, init_seed).items())
        self._weights_loaded = False     # still on the deterministic random initialisation (no checkpoint can be downloaded here)
        self.max_batch = int(max_batch)
        self._device: Optional[torch.device] = None
        self._engine = None
        self._engine_key = None
        self._debug = False

    # ---- nn.Module-like surface ----------------------------------------------------------------------------------
    def eval(self):
        return self

    def to(self, *args, **kwargs):
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, (torch.device, str)) and not isinstance(a, torch.dtype):
                dev = torch.device(a)
                if dev != self._device:
                    self._drop_engine()
                self._device = dev
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict(self._state)

    @staticmethod
    def _is_foreign(k: str) -> bool:
        raise NotImplementedError

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], strict: bool = True):
        new, seen = OrderedDict(), set()
        for k, v in sd.items():
            k = str(k)
            if self._is_foreign(k) or k in _METADATA_KEYS:
                continue
            if k not in self._spec:
                if strict:
                    raise RuntimeError(f"unexpected key {k!r} in CLIP state_dict")
                continue
            t = (v if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v))).detach().cpu().to(torch.float32)
            if tuple(t.shape) != tuple(self._spec[k]):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(t.shape)}, model {tuple(self._spec[k])}")
            new[k] = t.contiguous()
            seen.add(k)
        missing = [k for k in self._spec if k not in seen]
        if strict and missing:
            raise RuntimeError(f"missing keys in CLIP state_dict: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
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
            self._engine, self._engine_key = None, None

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _config(self, device_id: int):
        """The ctypes config struct of ``<_ABI>_create``."""
        raise NotImplementedError

    def _need_device(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}.{self._CALL} needs a HIP device ({self._INPUT} on 'cuda'); there is no CPU path")

    def _ensure_engine(self, device: torch.device):
        self._need_device(device)
        key = (device.index or 0, self.max_batch)
        if self._engine is not None and self._engine_key == key:
            return
        self._drop_engine()
        cc = self._config(device.index or 0)
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
        if self._debug:
            self._debug = False                     # (a failed allocation leaves the hook off)
            self.set_debug(True)

    def _engine_for(self, x: torch.Tensor) -> torch.device:
        """The start of an encode once the arguments are checked: the device (the input's, or the one ``to`` named for a host input), the
        random-weights notice, the engine."""
        dev = x.device if x.device.type == "cuda" else (self._device or x.device)
        self._need_device(dev)
        if not self._weights_loaded:
            self._weights_loaded = True             # (warn once per object)
            warnings.warn(f"{type(self).__name__} is encoding with its deterministic RANDOM initialisation: no CLIP state_dict was loaded "
                          "(load_state_dict); the embeddings carry no meaning", RuntimeWarning, stacklevel=3)
        self._ensure_engine(dev)
        return dev

    def _run(self, dev: torch.device, batch: int, call):
        """``call(entry, engine, b0, b1, stream)`` -> status, over ``batch`` samples at most ``max_batch`` at a time, on the current stream of ``dev``."""
        entry, stream = self._abi(self._CALL), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            for b0 in range(0, batch, self.max_batch):
                self._check(call(entry, self._engine, b0, min(batch, b0 + self.max_batch), stream), self._CALL)

    # ---- test hook: stage capture (include/tld_hip.h: tld_clip_set_debug, tld_clip_vis_set_debug) ---------------------
    def set_debug(self, on: bool = True):
        """Keep every stage of every block of the following encode calls (snapshot memory for ``max_batch`` samples is allocated here; a
        failure raises and leaves the hook off).  Before the engine exists the request is remembered and applied when it is built."""
        if self._engine is not None:
            self._check(self._abi("set_debug")(self._engine, int(bool(on))), "set_debug")
        self._debug = bool(on)

    def read_stage(self, name: str) -> torch.Tensor:
        """One stage of the engine's last encode call (the last chunk of a chunked encode), fp32 ``[rows, columns]`` on the host."""
        if self._engine is None:
            raise RuntimeError(f"read_stage: no engine yet ({self._CALL} first)")
        read = self._abi("read_stage")
        shape = (C.c_int64 * 4)()
        probe = np.empty(1, dtype=np.float32)
        rc = read(self._engine, name.encode(), probe.ctypes.data_as(C.POINTER(C.c_float)), -1, shape)
        if shape[0] == 0:                           # no such stage: the probe's own status says why
            self._check(rc or 1, f"read_stage({name})")
        out = np.empty((shape[0], shape[1]), dtype=np.float32)
        self._check(read(self._engine, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, shape), f"read_stage({name})")
        return torch.from_numpy(out)

    @property
    def weight_bytes(self) -> int:
        return int(self._abi("weight_bytes")(self._engine)) if self._engine is not None else 0


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


class ClipTextEncoder(_ClipEngine):
    _ABI, _CALL, _INPUT = "tld_clip", "encode_text", "tokens"

    def __init__(self, cfg: Optional[ClipTextConfig] = None, init_seed: int = 0, max_batch: int = 64):
        super().__init__(cfg if cfg is not None else ClipTextConfig(), clip_text_spec, synth_clip_state_dict, init_seed, max_batch)

    @staticmethod
    def _is_foreign(k: str) -> bool:
        return k.startswith("visual.")

    def _config(self, device_id: int):
        c = self.config
        return _lib.TldClipConfig(c.vocab_size, c.context_length, c.width, c.heads, c.layers, c.embed_dim, self.max_batch, device_id)

    @torch.no_grad()
    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        """``CLIP.encode_text(text)``: token ids ``[B, context_length]`` (any integer dtype) -> ``[B, embed_dim]`` fp32."""
        if text.dim() != 2 or text.shape[1] != self.config.context_length:
            raise ValueError(f"expected token ids [B, {self.config.context_length}], got {tuple(text.shape)}")
        dev = self._engine_for(text)
        tok = text.to(dev).to(torch.int32).contiguous()
        eot = tok.argmax(dim=-1).to(torch.int32).contiguous()            # clip/model.py: "take features from the eot embedding"
        out = torch.empty(tok.shape[0], self.config.embed_dim, dtype=torch.float32, device=dev)
        self._run(dev, tok.shape[0], lambda entry, eng, b0, b1, stream: entry(eng, _ptr(tok[b0:b1]), _ptr(eot[b0:b1]), _ptr(out[b0:b1]), b1 - b0, stream))
        return out


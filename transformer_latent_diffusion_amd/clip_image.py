"""``ClipImageEncoder``: CLIP's image tower on the gfx950 engine, and the CLIP score of generated pictures.

The denoiser's labels are CLIP ViT-L/14 *text* embeddings (tld/diffusion.py:136-140); the checkpoint ``clip.load`` returns holds the image
tower of the same joint space under ``visual.*``.  With that tower on the device, text-image alignment of an evaluation sample is
``cos(encode_image(decode(latents)), label)`` -- no text tower run, the label already is the text embedding.

    enc = ClipImageEncoder().load_state_dict(clip_state_dict).to("cuda")      # the full CLIP dict; the text side is ignored
    emb = enc.encode_image(clip_preprocess(images01, 224))                   # [B, 768] fp32
    scores = clip_score(emb, labels)                                         # [B] fp32, on the device

``Clip(text, visual)`` puts both towers behind one ``load_state_dict`` / ``to`` and is a drop-in for what ``clip.load`` returns wherever the
pipeline takes ``clip_model=``.  Arithmetic runs in ``libtld_hip.so`` (``tld_clip_vis_*``: restated ``VisionTransformer.forward`` of openai/CLIP
clip/model.py, bf16 MFMA projections and attention, fp32 residual stream / LayerNorm / softmax); there is no CPU path.  A fresh object holds
deterministic random weights (no checkpoint can be downloaded here).
"""
from __future__ import annotations

import ctypes as C
import warnings
from collections import OrderedDict
from dataclasses import dataclass
from typing import Mapping, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .clip_text import ClipTextEncoder, clip_text_spec

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)        # clip/clip.py _transform
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
_METADATA_KEYS = ("logit_scale", "input_resolution", "context_length", "vocab_size")


@dataclass
class ClipVisionConfig:
    """Vision-side fields of CLIP's constructor (defaults: ViT-L/14)."""
    image_size: int = 224         # image_resolution
    patch_size: int = 14          # vision_patch_size
    width: int = 1024             # vision_width
    heads: int = 16               # vision_width // 64
    layers: int = 24              # vision_layers
    embed_dim: int = 768

    @property
    def grid(self) -> int:
        return self.image_size // self.patch_size

    @property
    def tokens(self) -> int:
        return self.grid * self.grid + 1


def clip_visual_spec(cfg: ClipVisionConfig) -> "OrderedDict[str, Tuple[int, ...]]":
    """Ordered {key: shape} of the ``visual.*`` entries of ``CLIP.state_dict()`` (openai/CLIP clip/model.py, VisionTransformer)."""
    s: "OrderedDict[str, Tuple[int, ...]]" = OrderedDict()
    w = cfg.width
    s["visual.class_embedding"] = (w,)
    s["visual.positional_embedding"] = (cfg.tokens, w)
    s["visual.proj"] = (w, cfg.embed_dim)
    s["visual.conv1.weight"] = (w, 3, cfg.patch_size, cfg.patch_size)
    s["visual.ln_pre.weight"] = (w,)
    s["visual.ln_pre.bias"] = (w,)
    for i in range(cfg.layers):
        p = f"visual.transformer.resblocks.{i}."
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
    s["visual.ln_post.weight"] = (w,)
    s["visual.ln_post.bias"] = (w,)
    return s


def synth_clip_visual_state_dict(cfg: ClipVisionConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random image-tower weights (Philox): CLIP's own initialisation scales (clip/model.py VisionTransformer.__init__ and
    initialize_parameters) with non-trivial LayerNorm affines and biases and an in_proj that gives a peaked, not degenerate, softmax -- the recipe
    of ``synth_clip_state_dict``."""
    rng = np.random.Generator(np.random.Philox(key=seed + 0xC11F + 0x1000))
    w, L = cfg.width, cfg.layers
    scale = w ** -0.5
    proj_std, attn_std, fc_std = (w ** -0.5) * ((2 * L) ** -0.5), w ** -0.5, (2 * w) ** -0.5
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in clip_visual_spec(cfg).items():
        if k in ("visual.class_embedding", "visual.positional_embedding", "visual.proj"):
            v = scale * rng.standard_normal(shape)
        elif k == "visual.conv1.weight":
            v = (3 * cfg.patch_size ** 2) ** -0.5 * rng.standard_normal(shape)          # unit-variance patch features from unit-variance pixels
        elif ".ln_" in k:
            v = (1.0 + 0.2 * rng.standard_normal(shape)) if k.endswith("weight") else 0.1 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            v = 0.05 * rng.standard_normal(shape)
        elif "in_proj_weight" in k:
            v = 1.5 * attn_std * rng.standard_normal(shape)
        elif "out_proj.weight" in k or "c_proj.weight" in k:
            v = 4.0 * proj_std * rng.standard_normal(shape)
        else:
            v = fc_std * rng.standard_normal(shape)
        out[k] = np.asarray(v, dtype=np.float32)
    return out


def clip_visual_from_transformers(sd: Mapping[str, torch.Tensor]) -> "OrderedDict[str, torch.Tensor]":
    """``transformers`` ``CLIPVisionModelWithProjection.state_dict()`` (or the vision side of ``CLIPModel``'s) under the OpenAI names: the q / k / v
    projections concatenated into ``in_proj``, ``visual_projection.weight`` transposed into ``visual.proj`` (upstream spells ``pre_layrnorm``).
    Entries of other parts of a ``CLIPModel`` are left out."""
    out: "OrderedDict[str, torch.Tensor]" = OrderedDict()
    g = lambda k: sd[k].detach().to(torch.float32)
    vm = "vision_model."
    out["visual.class_embedding"] = g(vm + "embeddings.class_embedding")
    out["visual.positional_embedding"] = g(vm + "embeddings.position_embedding.weight")
    out["visual.proj"] = g("visual_projection.weight").t().contiguous()
    out["visual.conv1.weight"] = g(vm + "embeddings.patch_embedding.weight")
    for n in ("weight", "bias"):
        out[f"visual.ln_pre.{n}"] = g(vm + f"pre_layrnorm.{n}")
    layers = sorted({int(k.split(".")[3]) for k in sd if k.startswith(vm + "encoder.layers.")})
    names = {"ln_1": "layer_norm1", "ln_2": "layer_norm2", "attn.out_proj": "self_attn.out_proj", "mlp.c_fc": "mlp.fc1", "mlp.c_proj": "mlp.fc2"}
    for i in layers:
        src, dst = vm + f"encoder.layers.{i}.", f"visual.transformer.resblocks.{i}."
        for n in ("weight", "bias"):
            out[dst + f"attn.in_proj_{n}"] = torch.cat([g(src + f"self_attn.{p}_proj.{n}") for p in "qkv"], dim=0)
            for ours, theirs in names.items():
                out[dst + f"{ours}.{n}"] = g(src + f"{theirs}.{n}")
    for n in ("weight", "bias"):
        out[f"visual.ln_post.{n}"] = g(vm + f"post_layernorm.{n}")
    return out


def clip_preprocess(images, size: int = 224) -> torch.Tensor:
    """CLIP's ``_transform(size)`` (clip/clip.py): bicubic resize of the shorter side to ``size``, centre crop, [0, 1], normalise with CLIP's
    mean / std.  Returns ``[B, 3, size, size]`` fp32.

    * a PIL image or a sequence of them: PIL's own bicubic resize, exactly upstream (result on the CPU);
    * a float tensor ``[B, 3, H, W]`` in [0, 1] on any device: ``F.interpolate(mode="bicubic", antialias=True)`` of the shorter side, centre
      crop, clamp to [0, 1], normalise -- everything stays on the tensor's device.  This is NOT bit-equal to the PIL path (PIL resizes 8-bit
      pixels with its own fixed-point filter).  An input already ``size x size`` is only normalised: ``(x - mean) / std``.
    """
    if not isinstance(images, torch.Tensor):
        from PIL import Image
        if isinstance(images, Image.Image):
            images = [images]
        out = []
        for im in images:
            w, h = im.size
            if (w, h) != (size, size):
                # torchvision Resize(size): the shorter side becomes size, the longer int(size * long / short)
                nw, nh = (size, int(size * h / w)) if w <= h else (int(size * w / h), size)
                im = im.resize((nw, nh), Image.BICUBIC)
                left, top = int(round((nw - size) / 2.0)), int(round((nh - size) / 2.0))      # torchvision CenterCrop
                im = im.crop((left, top, left + size, top + size))
            a = np.asarray(im.convert("RGB"), dtype=np.float32) / 255.0
            out.append(torch.from_numpy(a).permute(2, 0, 1))
        x = torch.stack(out)
    else:
        x = images
        if x.dim() != 4 or x.shape[1] != 3 or not x.is_floating_point():
            raise ValueError(f"clip_preprocess: expected a float tensor [B, 3, H, W] in [0, 1], got {tuple(x.shape)} {x.dtype}")
        x = x.to(torch.float32)
        h, w = x.shape[-2:]
        if (h, w) != (size, size):
            nh, nw = (int(size * h / w), size) if w <= h else (size, int(size * w / h))
            x = F.interpolate(x, size=(nh, nw), mode="bicubic", antialias=True, align_corners=False)
            top, left = int(round((nh - size) / 2.0)), int(round((nw - size) / 2.0))
            x = x[:, :, top:top + size, left:left + size].clamp(0.0, 1.0)
    mean = torch.tensor(CLIP_MEAN, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=torch.float32, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def clip_score(image_emb: torch.Tensor, text_emb: torch.Tensor) -> torch.Tensor:
    """Per-pair cosine similarity of ``[B, E]`` image and text embeddings: ``[B]`` fp32 on the inputs' device.  A zero vector gives 0, not NaN."""
    if image_emb.shape != text_emb.shape or image_emb.dim() != 2:
        raise ValueError(f"clip_score: expected two [B, E] tensors, got {tuple(image_emb.shape)} and {tuple(text_emb.shape)}")
    a, b = image_emb.to(torch.float32), text_emb.to(device=image_emb.device, dtype=torch.float32)
    den = a.norm(dim=-1) * b.norm(dim=-1)
    dot = (a * b).sum(dim=-1)
    return torch.where(den > 0, dot / den.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(dot))


_IO_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


class ClipImageEncoder:
    def __init__(self, cfg: Optional[ClipVisionConfig] = None, init_seed: int = 0, max_batch: int = 16):
        self.config = cfg if cfg is not None else ClipVisionConfig()
        if self.config.heads * 64 != self.config.width:
            raise ValueError("head_dim must be 64 (width // heads)")
        self._spec = clip_visual_spec(self.config)
        self._state: "OrderedDict[str, torch.Tensor]" = OrderedDict(
            (k, torch.from_numpy(v)) for k, v in synth_clip_visual_state_dict(self.config, init_seed).items())
        self._weights_loaded = False     # still on the deterministic random initialisation (no checkpoint can be downloaded here)
        self.max_batch = int(max_batch)
        self._device: Optional[torch.device] = None
        self._engine = None
        self._engine_key = None
        self._debug = False

    @property
    def input_resolution(self) -> int:
        """``model.visual.input_resolution`` of openai/CLIP."""
        return self.config.image_size

    # ---- nn.Module-like surface ----------------------------------------------------------------------------------
    def eval(self) -> "ClipImageEncoder":
        return self

    def to(self, *args, **kwargs) -> "ClipImageEncoder":
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
    def _is_text_key(k: str) -> bool:
        return (k in ("token_embedding.weight", "positional_embedding", "text_projection") or k.startswith("ln_final.") or
                k.startswith("transformer.resblocks."))

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], strict: bool = True) -> "ClipImageEncoder":
        new, seen = OrderedDict(), set()
        for k, v in sd.items():
            k = str(k)
            if self._is_text_key(k) or k in _METADATA_KEYS:
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
    def _drop_engine(self):
        if self._engine is not None:
            _lib.lib().tld_clip_vis_destroy(self._engine)
            self._engine, self._engine_key = None, None

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _ensure_engine(self, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError("ClipImageEncoder.encode_image needs a HIP device (pixels on 'cuda'); there is no CPU path")
        key = (device.index or 0, self.max_batch)
        if self._engine is not None and self._engine_key == key:
            return
        self._drop_engine()
        L, c = _lib.lib(), self.config
        cc = _lib.TldClipVisConfig(c.image_size, c.patch_size, c.width, c.heads, c.layers, c.embed_dim, self.max_batch, device.index or 0)
        h = C.c_void_p()
        _lib.check(L.tld_clip_vis_create(C.byref(cc), C.byref(h)), "tld_clip_vis_create")
        try:
            for k, t in self._state.items():
                a = np.ascontiguousarray(t.numpy(), dtype=np.float32)
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(L.tld_clip_vis_load_tensor(h, k.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, _lib.DTYPE_F32),
                           f"tld_clip_vis_load_tensor({k})")
            _lib.check(L.tld_clip_vis_finalize_weights(h), "tld_clip_vis_finalize_weights")
        except Exception:
            L.tld_clip_vis_destroy(h)
            raise
        self._engine, self._engine_key = h, key
        if self._debug:
            self._debug = False                     # (a failed allocation leaves the hook off)
            self.set_debug(True)

    # ---- test hook: stage capture (include/tld_hip.h: tld_clip_vis_set_debug) ----------------------------------------
    def set_debug(self, on: bool = True):
        """Keep every stage of every block of the following encode_image calls (snapshot memory for ``max_batch`` images is allocated here; a
        failure raises and leaves the hook off).  Before the engine exists the request is remembered and applied when it is built."""
        if self._engine is not None:
            _lib.check(_lib.lib().tld_clip_vis_set_debug(self._engine, int(bool(on))), "tld_clip_vis_set_debug")
        self._debug = bool(on)

    def read_stage(self, name: str) -> torch.Tensor:
        """One stage of the last ``tld_clip_vis_encode_image`` call (the last chunk of a chunked encode), fp32 ``[rows, columns]`` on the host."""
        if self._engine is None:
            raise RuntimeError("read_stage: no engine yet (encode_image first)")
        read = _lib.lib().tld_clip_vis_read_stage
        shape = (C.c_int64 * 4)()
        probe = np.empty(1, dtype=np.float32)
        rc = read(self._engine, name.encode(), probe.ctypes.data_as(C.POINTER(C.c_float)), -1, shape)
        if shape[0] == 0:                           # no such stage: the probe's own status says why
            _lib.check(rc or 1, f"tld_clip_vis_read_stage({name})")
        out = np.empty((shape[0], shape[1]), dtype=np.float32)
        _lib.check(read(self._engine, name.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, shape), f"tld_clip_vis_read_stage({name})")
        return torch.from_numpy(out)

    @torch.no_grad()
    def encode_image(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``CLIP.encode_image(image)``: normalised pixels ``[B, 3, R, R]`` (fp32, fp16 or bf16; what ``clip_preprocess`` returns) ->
        ``[B, embed_dim]`` fp32 on the pixels' device."""
        R = self.config.image_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, R, R):
            raise ValueError(f"expected pixels [B, 3, {R}, {R}], got {tuple(pixel_values.shape)}")
        if pixel_values.dtype not in _IO_DTYPES:
            raise ValueError(f"expected fp32, fp16 or bf16 pixels, got {pixel_values.dtype}")
        dev = pixel_values.device if pixel_values.device.type == "cuda" else (self._device or pixel_values.device)
        if dev.type != "cuda":
            raise RuntimeError("ClipImageEncoder.encode_image needs a HIP device (pixels on 'cuda'); there is no CPU path")
        if not self._weights_loaded:
            self._weights_loaded = True             # (warn once per object)
            warnings.warn("ClipImageEncoder is encoding with its deterministic RANDOM initialisation: no CLIP state_dict was loaded "
                          "(load_state_dict); the embeddings carry no meaning", RuntimeWarning, stacklevel=2)
        self._ensure_engine(dev)
        pix = pixel_values.to(dev).contiguous()
        B = pix.shape[0]
        out = torch.empty(B, self.config.embed_dim, dtype=torch.float32, device=dev)
        L = _lib.lib()
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            for b0 in range(0, B, self.max_batch):
                b1 = min(B, b0 + self.max_batch)
                _lib.check(L.tld_clip_vis_encode_image(self._engine, C.c_void_p(pix[b0:b1].data_ptr()), C.c_void_p(out[b0:b1].data_ptr()), b1 - b0,
                                                       _IO_DTYPES[pix.dtype], C.c_void_p(stream)), "tld_clip_vis_encode_image")
        return out

    @property
    def weight_bytes(self) -> int:
        return int(_lib.lib().tld_clip_vis_weight_bytes(self._engine)) if self._engine is not None else 0


class Clip:
    """Both towers behind one ``load_state_dict`` / ``to``: what ``clip.load`` returns, as far as the pipeline uses it (``encode_text``,
    ``encode_image``, ``visual.input_resolution``).  ``vae.AutoencoderKL`` pairs its two engines the same way."""

    def __init__(self, text: Optional[ClipTextEncoder] = None, visual: Optional[ClipImageEncoder] = None):
        self.text = text if text is not None else ClipTextEncoder()
        self.visual = visual if visual is not None else ClipImageEncoder()

    def eval(self) -> "Clip":
        return self

    def to(self, *args, **kwargs) -> "Clip":
        self.text.to(*args, **kwargs)
        self.visual.to(*args, **kwargs)
        return self

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        sd = self.text.state_dict()
        sd.update(self.visual.state_dict())
        return sd

    def load_state_dict(self, sd: Mapping[str, torch.Tensor], strict: bool = True) -> "Clip":
        if strict:                                  # each tower skips the other's keys by name; what neither knows is unexpected
            known = set(clip_text_spec(self.text.config)) | set(self.visual._spec) | set(_METADATA_KEYS)
            extra = [str(k) for k in sd if str(k) not in known]
            if extra:
                raise RuntimeError(f"unexpected key {extra[0]!r} in CLIP state_dict")
        self.text.load_state_dict(sd, strict=strict)
        self.visual.load_state_dict(sd, strict=strict)
        return self

    def parameters(self):
        yield from self.text.parameters()
        yield from self.visual.parameters()

    def encode_text(self, text: torch.Tensor) -> torch.Tensor:
        return self.text.encode_text(text)

    def encode_image(self, pixel_values: torch.Tensor) -> torch.Tensor:
        return self.visual.encode_image(pixel_values)

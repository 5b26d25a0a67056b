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

from collections import OrderedDict
from dataclasses import dataclass
from typing import Mapping, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib
from .clip_text import (_METADATA_KEYS, ClipTextEncoder, _block_spec, _ClipEngine, _ptr, _synth_transformer_entry, clip_text_spec)

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)        # clip/clip.py _transform
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


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
    _block_spec(s, "visual.transformer.resblocks.", cfg.layers, w)
    s["visual.ln_post.weight"] = (w,)
    s["visual.ln_post.bias"] = (w,)
    return s


def synth_clip_visual_state_dict(cfg: ClipVisionConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    """Deterministic random image-tower weights (Philox): CLIP's own initialisation scales (clip/model.py VisionTransformer.__init__ and
    initialize_parameters) with non-trivial LayerNorm affines and biases and an in_proj that gives a peaked, not degenerate, softmax -- the recipe
    of ``synth_clip_state_dict``."""
    rng = np.random.Generator(np.random.Philox(key=seed + 0xC11F + 0x1000))
    w = cfg.width
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    for k, shape in clip_visual_spec(cfg).items():
        if k in ("visual.class_embedding", "visual.positional_embedding", "visual.proj"):
            v = w ** -0.5 * rng.standard_normal(shape)
        elif k == "visual.conv1.weight":
            v = (3 * cfg.patch_size ** 2) ** -0.5 * rng.standard_normal(shape)          # unit-variance patch features from unit-variance pixels
        else:
            v = _synth_transformer_entry(rng, k, shape, w, cfg.layers)
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


class ClipImageEncoder(_ClipEngine):
    _ABI, _CALL, _INPUT = "tld_clip_vis", "encode_image", "pixels"

    def __init__(self, cfg: Optional[ClipVisionConfig] = None, init_seed: int = 0, max_batch: int = 16):
        super().__init__(cfg if cfg is not None else ClipVisionConfig(), clip_visual_spec, synth_clip_visual_state_dict, init_seed, max_batch)

    @property
    def input_resolution(self) -> int:
        """``model.visual.input_resolution`` of openai/CLIP."""
        return self.config.image_size

    @staticmethod
    def _is_foreign(k: str) -> bool:
        return (k in ("token_embedding.weight", "positional_embedding", "text_projection") or k.startswith("ln_final.") or
                k.startswith("transformer.resblocks."))

    def _config(self, device_id: int):
        c = self.config
        return _lib.TldClipVisConfig(c.image_size, c.patch_size, c.width, c.heads, c.layers, c.embed_dim, self.max_batch, device_id)

    @torch.no_grad()
    def encode_image(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``CLIP.encode_image(image)``: normalised pixels ``[B, 3, R, R]`` (fp32, fp16 or bf16; what ``clip_preprocess`` returns) ->
        ``[B, embed_dim]`` fp32 on the pixels' device."""
        R = self.config.image_size
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != (3, R, R):
            raise ValueError(f"expected pixels [B, 3, {R}, {R}], got {tuple(pixel_values.shape)}")
        if pixel_values.dtype not in _IO_DTYPES:
            raise ValueError(f"expected fp32, fp16 or bf16 pixels, got {pixel_values.dtype}")
        dev = self._engine_for(pixel_values)
        pix = pixel_values.to(dev).contiguous()
        out = torch.empty(pix.shape[0], self.config.embed_dim, dtype=torch.float32, device=dev)
        self._run(dev, pix.shape[0], lambda entry, eng, b0, b1, stream: entry(eng, _ptr(pix[b0:b1]), _ptr(out[b0:b1]), b1 - b0, _IO_DTYPES[pix.dtype], stream))
        return out


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

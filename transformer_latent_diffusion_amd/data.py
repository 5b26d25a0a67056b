"""The training data path on the device: the reference's stored formats (tld/data.py -- latents as uint8 codes of
``quantize_latents`` or as fp16, text embeddings as fp16) held resident in device memory, batches addressed by a device index vector and built by
one kernel (``Trainer.prepare_batch`` -> ``tld_train_prepare_batch``).  A million 256 px images are 4 KB of codes + 1.5 KB of embedding each."""
from __future__ import annotations

import ctypes as C
from typing import Iterator

import torch

from . import _lib

_LATENT_DTYPES = {torch.uint8: _lib.DTYPE_U8, torch.float16: _lib.DTYPE_F16, torch.float32: _lib.DTYPE_F32}
_LABEL_DTYPES = {torch.float16: _lib.DTYPE_F16, torch.float32: _lib.DTYPE_F32}


def quantize_latents(lat: torch.Tensor, clip_val: float = 20) -> torch.Tensor:
    """tld/data.py:52-55: clip to +-clip_val, map to [0, 255], truncate to uint8."""
    lat_norm = lat.clip(-clip_val, clip_val) / clip_val
    return (((lat_norm + 1) / 2) * 255).to(torch.uint8)


def dequantize_latents(lat: torch.Tensor, clip_val: float = 20) -> torch.Tensor:
    """tld/data.py:58-60: the fp16 value of a code (every step in fp16, as there)."""
    lat_norm = (lat.to(torch.float16) / 255) * 2 - 1
    return lat_norm * clip_val


class DeviceLatentDataset:
    """``latents`` [rows, C, S, S] (uint8 codes, fp16 or fp32, UNscaled as the reference stores them) and ``text_emb`` [rows, text_emb] (fp16 or fp32),
    moved to ``device`` once.  What a training step sees of row r is ``dequantize_latents(code).float() / vae_scale_factor`` for codes (a 256-entry
    table built here on the host) and ``float(latent) / vae_scale_factor`` otherwise -- the loader's batch after tld/train.py:122."""

    def __init__(self, latents: torch.Tensor, text_emb: torch.Tensor, *, clip_val: float = 20, vae_scale_factor: float = 8, device):
        if not (isinstance(latents, torch.Tensor) and isinstance(text_emb, torch.Tensor)):
            raise TypeError("latents and text_emb must be torch tensors")
        if latents.dtype not in _LATENT_DTYPES:
            raise TypeError(f"latents are {latents.dtype}: uint8, float16 or float32")
        if text_emb.dtype not in _LABEL_DTYPES:
            raise TypeError(f"text_emb is {text_emb.dtype}: float16 or float32")
        if latents.dim() < 2 or text_emb.dim() != 2 or latents.shape[0] != text_emb.shape[0] or latents.shape[0] == 0:
            raise ValueError(f"latents {tuple(latents.shape)} and text_emb {tuple(text_emb.shape)}: [rows, ...] and [rows, text_emb] with the same rows > 0")
        if not float(vae_scale_factor) > 0 or not float(clip_val) > 0:
            raise ValueError("clip_val and vae_scale_factor must be positive")
        self.device = torch.device(device)
        self.clip_val, self.vae_scale_factor = float(clip_val), float(vae_scale_factor)
        self.latents = latents.detach().to(self.device).contiguous()
        self.text_emb = text_emb.detach().to(self.device).contiguous()
        self.sample_shape = tuple(self.latents.shape[1:])
        self.latent_elems = int(self.latents[0].numel())
        self.table = None
        if latents.dtype == torch.uint8:
            self.table = (dequantize_latents(torch.arange(256), self.clip_val).float() / self.vae_scale_factor).to(self.device)

    def __len__(self) -> int:
        return int(self.latents.shape[0])

    def batches(self, batch_size: int, seed: int = 0, epoch: int = 0) -> Iterator[torch.Tensor]:
        """Index slices of one device ``randperm`` per (seed, epoch): a shuffled pass over the rows; the last batch may be short, as with the
        reference's ``DataLoader`` (tld/train.py:80, drop_last off)."""
        if batch_size <= 0:
            raise ValueError("batch_size must be positive")
        g = torch.Generator(device=self.device)
        g.manual_seed((int(seed) * 0x9E3779B97F4A7C15 + int(epoch)) & (2 ** 63 - 1))
        perm = torch.randperm(len(self), generator=g, device=self.device)
        for i in range(0, len(self), batch_size):
            yield perm[i:i + batch_size]

    def source(self) -> "_lib.TldBatchSource":
        """The C descriptor of this dataset (pointers into the tensors this object keeps alive)."""
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return _lib.TldBatchSource(p(self.latents), p(self.text_emb), p(self.table), len(self), _LATENT_DTYPES[self.latents.dtype],
                                   _LABEL_DTYPES[self.text_emb.dtype], self.latent_elems, int(self.text_emb.shape[1]), self.vae_scale_factor)

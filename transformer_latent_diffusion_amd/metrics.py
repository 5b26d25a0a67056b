"""Distribution metrics on CLIP image embeddings, computed on the device: the Frechet distance on CLIP features (FID's
formula on what ``ClipImageEncoder.encode_image`` returns) and CMMD (Jayasumana et al., "Rethinking FID", 2024: the squared maximum mean
discrepancy with a Gaussian kernel, sigma = 10, on L2-normalised embeddings, times 1000).

    real, fake = FeatureBank(768, 30000, dev), FeatureBank(768, 30000, dev)
    for batch in real_images:  pipeline.image_features(batch, bank=real)            # DiffusionTransformer.image_features
    for labels, seed in plan:  trainer.eval_features(labels, vae, clip, fake, seed=seed)
    cmmd(real, fake), frechet_distance(real, fake)
    real.moments().save("real_stats.npz")                                           # the "FID statistics file" workflow

The embeddings never leave the device: ``FeatureBank.add`` is one kernel (``tld_feat_append``), the moments are two (``tld_feat_moments``) and every
pair sum is ``tld_feat_kernel_sum`` on the exact-fp32 MFMA.  There is no fallback: without the library or a HIP device these raise.

One rank only: a bank holds what its own process added.  Gathering banks across ranks is ``torch.distributed`` plumbing (an ``all_gather`` of
``bank.features()`` into a larger bank) and is not done here.

No value of these metrics has been checked against published CLIP-FD or CMMD numbers: the ViT-L/14@336 tower the CMMD paper uses is outside the image
tower's 257-token limit, so values from the 224 px tower compare with each other, not with the paper's.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Union

import numpy as np
import torch

from . import _lib

MAX_DIM = 4096                      # FEAT_MAX_DIM (csrc/tld_feat_plan.h)
CMMD_SIGMA, CMMD_SCALE = 10.0, 1000.0

_IO_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


def feat_pitch(dim: int) -> int:
    """Columns of a bank row: ``dim`` rounded up to a multiple of 32 (feat_pitch, csrc/tld_feat_plan.h)."""
    return (int(dim) + 31) // 32 * 32


def _ptr(t: torch.Tensor) -> C.c_void_p:
    return C.c_void_p(t.data_ptr())


@dataclass
class FeatureMoments:
    """``n`` rows' mean ``[dim]`` and sample covariance ``[dim, dim]`` (ddof = 1), float64 tensors -- what a Frechet distance needs of a set."""
    n: int
    mean: torch.Tensor
    cov: torch.Tensor

    def cpu(self) -> "FeatureMoments":
        return FeatureMoments(int(self.n), self.mean.detach().cpu(), self.cov.detach().cpu())

    def save(self, path) -> None:
        """A plain ``.npz`` with ``n``, ``mean`` and ``cov``."""
        m = self.cpu()
        with open(path, "wb") as f:
            np.savez(f, n=np.int64(m.n), mean=m.mean.numpy(), cov=m.cov.numpy())

    @staticmethod
    def load(path) -> "FeatureMoments":
        with np.load(path) as z:
            mean, cov = np.asarray(z["mean"], dtype=np.float64), np.asarray(z["cov"], dtype=np.float64)
            n = int(z["n"])
        if mean.ndim != 1 or cov.shape != (mean.shape[0], mean.shape[0]):
            raise ValueError(f"FeatureMoments.load: mean {mean.shape} and cov {cov.shape} do not belong together")
        return FeatureMoments(n, torch.from_numpy(mean), torch.from_numpy(cov))


class FeatureBank:
    """``capacity`` embeddings of width ``dim`` as a device fp32 matrix ``[capacity, pitch]`` (pad columns zero).  ``normalize=True`` stores every
    row divided by its L2 norm (formed in double, rounded once), which is what CMMD is defined on; a row with norm 0 or a non-finite value is stored
    as zeros and counted (``bad_rows``), the idea of ``Trainer.bad_indices``."""

    def __init__(self, dim: int, capacity: int, device, normalize: bool = True):
        dim, capacity = int(dim), int(capacity)
        if not 1 <= dim <= MAX_DIM:
            raise ValueError(f"FeatureBank: dim {dim} outside [1, {MAX_DIM}]")
        if capacity < 1:
            raise ValueError(f"FeatureBank: capacity {capacity}")
        self.dim, self.capacity, self.pitch, self.normalize = dim, capacity, feat_pitch(dim), bool(normalize)
        self.device = torch.device(device)
        self._data = torch.zeros(capacity, self.pitch, dtype=torch.float32, device=self.device)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._n = 0

    def __len__(self) -> int:
        return self._n

    def _need_device(self, what: str) -> None:
        if self.device.type != "cuda":
            raise RuntimeError(f"FeatureBank.{what} needs a HIP device (the bank is on {self.device}); there is no CPU path")

    def add(self, emb: torch.Tensor) -> "FeatureBank":
        """Append ``emb`` ``[rows, dim]`` (fp32, fp16 or bf16).  One kernel on the current stream, no host synchronisation: the row count is the
        host's.  Raises past ``capacity``."""
        if emb.dim() != 2 or emb.shape[1] != self.dim:
            raise ValueError(f"FeatureBank.add: expected [rows, {self.dim}], got {tuple(emb.shape)}")
        if emb.dtype not in _IO_DTYPES:
            raise ValueError(f"FeatureBank.add: expected fp32, fp16 or bf16 embeddings, got {emb.dtype}")
        rows = int(emb.shape[0])
        if rows == 0:
            return self
        if self._n + rows > self.capacity:
            raise ValueError(f"FeatureBank.add: {rows} rows past {self._n} do not fit the capacity {self.capacity}")
        self._need_device("add")
        src = emb.detach().to(self.device).contiguous()
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().tld_feat_append(_ptr(self._data), self.capacity, self._n, self.dim, self.pitch, _ptr(src), _IO_DTYPES[src.dtype], rows,
                                                  int(self.normalize), _ptr(self._bad), C.c_void_p(stream)), "tld_feat_append")
        self._n += rows
        return self

    def features(self) -> torch.Tensor:
        """The used rows, ``[len, dim]``: a view of the bank (row stride ``pitch``), not a copy."""
        return self._data[:self._n, :self.dim]

    def bad_rows(self) -> int:
        """Rows stored as zeros because their norm was 0 or a value was not finite.  Synchronises."""
        return int(self._bad.item())

    def moments(self) -> FeatureMoments:
        """``numpy.mean(axis=0)`` and ``numpy.cov(rowvar=False)`` of the used rows as float64 device tensors (``tld_feat_moments``)."""
        self._need_device("moments")
        mean = torch.empty(self.dim, dtype=torch.float64, device=self.device)
        cov = torch.empty(self.dim, self.dim, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device).cuda_stream
            _lib.check(_lib.lib().tld_feat_moments(_ptr(self._data), self._n, self.dim, self.pitch, _ptr(mean), _ptr(cov), C.c_void_p(stream)),
                       "tld_feat_moments")
        return FeatureMoments(self._n, mean, cov)


def _as_moments(x: Union[FeatureBank, FeatureMoments]) -> FeatureMoments:
    if isinstance(x, FeatureMoments):
        return x
    if isinstance(x, FeatureBank):
        return x.moments()
    raise TypeError(f"expected a FeatureBank or FeatureMoments, got {type(x).__name__}")


def frechet_distance(a: Union[FeatureBank, FeatureMoments], b: Union[FeatureBank, FeatureMoments]) -> float:
    """``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr (S1 S2)^(1/2)`` of two banks or moment sets: FID's formula (Heusel et al. 2017) on whatever features
    they hold.  Host numpy float64 on the two moment sets (a one-off on dim x dim; this copies them and so synchronises).  The trace of the matrix
    square root is ``sum_k sqrt(lambda_k)`` with ``lambda = eigvalsh(R S2 R)``, ``R = S1^(1/2)`` by ``eigh``, eigenvalues clipped at 0: symmetric
    real arithmetic throughout, no ``sqrtm``.  Below ``dim`` samples the covariances are rank-deficient and the value says little, as for FID."""
    ma, mb = _as_moments(a).cpu(), _as_moments(b).cpu()
    mu1, s1, mu2, s2 = ma.mean.numpy(), ma.cov.numpy(), mb.mean.numpy(), mb.cov.numpy()
    if mu1.shape != mu2.shape or s1.shape != s2.shape:
        raise ValueError(f"frechet_distance: widths {mu1.shape[0]} and {mu2.shape[0]}")
    w, v = np.linalg.eigh((s1 + s1.T) * 0.5)
    root = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    inner = root @ ((s2 + s2.T) * 0.5) @ root
    lam = np.clip(np.linalg.eigvalsh((inner + inner.T) * 0.5), 0.0, None)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(lam).sum())


def kernel_sum(a: FeatureBank, b: FeatureBank, gamma: float) -> torch.Tensor:
    """``sum_ij expm1(-gamma |a_i - b_j|^2)`` over the used rows of two banks as a 0-d float64 device tensor (``tld_feat_kernel_sum``); ``b is a``
    runs the same-set form, whose terms i == j are exactly 0.  Not synchronised."""
    if a.dim != b.dim or a.device != b.device:
        raise ValueError(f"kernel_sum: banks of width {a.dim} on {a.device} and width {b.dim} on {b.device}")
    a._need_device("kernel_sum")
    same = int(a is b)
    L = _lib.lib()
    count = int(L.tld_feat_kernel_sum_partials(len(a), len(b), same))
    if count < 1:
        raise ValueError(f"kernel_sum: {len(a)} and {len(b)} rows (at least one each)")
    partials = torch.empty(count, dtype=torch.float64, device=a.device)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        _lib.check(L.tld_feat_kernel_sum(_ptr(a._data), len(a), _ptr(b._data), len(b), a.dim, a.pitch, float(gamma), same, _ptr(partials), count, _ptr(out),
                                         C.c_void_p(stream)), "tld_feat_kernel_sum")
    return out[0]


def mmd2(a: FeatureBank, b: FeatureBank, sigma: float = 10.0, unbiased: bool = False) -> torch.Tensor:
    """Squared maximum mean discrepancy of two banks under ``k(x, y) = exp(-|x - y|^2 / (2 sigma^2))``, from three pair sums of ``k - 1`` (the ones
    cancel exactly in both estimators, and dropping them before rounding keeps the digits of what is left):

        biased (the published CMMD code's):  S_xx / n^2 + S_yy / m^2 - 2 S_xy / (n m)
        unbiased:                            S_xx / (n (n - 1)) + S_yy / (m (m - 1)) - 2 S_xy / (n m)

    with the same three sums, since the i == j terms of ``k - 1`` are exactly 0.  Returns a 0-d float64 device tensor, not synchronised."""
    sigma = float(sigma)
    if not (sigma > 0.0):
        raise ValueError(f"mmd2: sigma {sigma}")
    n, m = len(a), len(b)
    if n < 1 or m < 1 or (unbiased and (n < 2 or m < 2)):
        raise ValueError(f"mmd2: {n} and {m} rows")
    gamma = 1.0 / (2.0 * sigma * sigma)
    sxx, syy, sxy = kernel_sum(a, a, gamma), kernel_sum(b, b, gamma), kernel_sum(a, b, gamma)
    dx, dy = (n * (n - 1), m * (m - 1)) if unbiased else (n * n, m * m)
    return sxx / float(dx) + syy / float(dy) - 2.0 * sxy / float(n * m)


def cmmd(a: FeatureBank, b: FeatureBank) -> torch.Tensor:
    """CMMD: ``1000 * mmd2(a, b, sigma=10)``, biased, on L2-normalised embeddings.  Refuses a bank built with ``normalize=False``."""
    for x in (a, b):
        if not isinstance(x, FeatureBank):
            raise TypeError(f"cmmd: expected FeatureBanks, got {type(x).__name__}")
        if not x.normalize:
            raise ValueError("cmmd is defined on L2-normalised embeddings: build the bank with normalize=True")
    return CMMD_SCALE * mmd2(a, b, CMMD_SIGMA)


def image_embeddings(clip_image, images01: torch.Tensor, device) -> torch.Tensor:
    """``clip_image.encode_image(clip_preprocess(images01))`` for a float tensor ``[B, 3, H, W]`` in [0, 1] (or PIL images): the chain
    ``Trainer.eval_clip_score`` and ``DiffusionTransformer.clip_scores`` run.  ``clip_image``: a ``ClipImageEncoder`` or a ``Clip``."""
    from .clip_image import clip_preprocess
    size = getattr(clip_image, "visual", clip_image).input_resolution
    if isinstance(images01, torch.Tensor):
        images01 = images01.to(device, torch.float32)
    return clip_image.encode_image(clip_preprocess(images01, size).to(device))

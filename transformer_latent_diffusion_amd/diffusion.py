"""Sampler and pipeline surface: ``DiffusionGenerator`` and ``DiffusionTransformer``.

Same signatures, defaults and return values as the reference (tld/diffusion.py:22-125, :143-186);
the reverse-diffusion loop itself (CFG doubled batch, DPM-Solver++(2M) / DDIM update, final
prediction, latent shifts) runs on the device inside ``tld_sample`` -- Python computes the float64
schedule scalars (schedule.py), draws or accepts the initial noise, and hands off to the VAE at
the exit edge.  CLIP and the VAE are third-party models outside the denoising path: they are injected
(or imported lazily when installed) and never re-implemented here.
"""
from __future__ import annotations

import numbers
import os
from dataclasses import asdict, dataclass
from typing import Any, NamedTuple, Optional

import numpy as np
import torch
from torch import Tensor

from . import schedule
from .configs import LTDConfig
from .denoiser import Denoiser

device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")


def check_mask_range(mask: Tensor, meaning: str = ""):
    """An inpainting mask holds values in [0, 1]; ``meaning`` ends the message."""
    if mask.numel():
        lo, hi = float(mask.min()), float(mask.max())
        if not (lo >= 0.0 and hi <= 1.0):
            raise ValueError(f"mask values span [{lo}, {hi}]: expected [0, 1]{meaning}")


def stack_optional(v, what: str, B: int, shape: tuple, fill: float):
    """A per-request optional operand as one tensor: ``v`` is None, a tensor [B, *shape] (returned as it is) or a length-B sequence of
    [*shape] tensors / None; returns None where no entry is given, else fp32 [B, *shape] on the host with ``fill`` for the None entries."""
    if v is None or isinstance(v, Tensor):
        if v is not None and tuple(v.shape) != (B,) + shape:
            raise ValueError(f"{what} {tuple(v.shape)}: expected {(B,) + shape}")
        return v
    v = list(v)
    if len(v) != B:
        raise ValueError(f"{what}: {len(v)} entries for {B} requests")
    if all(t is None for t in v):
        return None
    for b, t in enumerate(v):
        if t is not None and tuple(t.shape) != shape:
            raise ValueError(f"{what}[{b}] {tuple(t.shape)}: expected {shape}")
    return torch.stack([torch.full(shape, fill) if t is None else t.detach().to("cpu", torch.float32) for t in v])


def per_request_intervals(v, B: int):
    """``guidance_interval`` as one entry per request: ``v`` is None, one ``(lo, hi)`` pair of numbers (for all), or a length-B sequence of
    pairs / None (a request without one is guided throughout).  Returns a list of B ``(lo, hi)`` float pairs / None; ``lo > hi`` raises."""
    if v is None:
        return [None] * B
    v = list(v)
    if len(v) == 2 and all(isinstance(x, numbers.Number) for x in v):
        v = [tuple(v)] * B
    if len(v) != B:
        raise ValueError(f"guidance_interval: {len(v)} entries for {B} requests")
    out = []
    for b, iv in enumerate(v):
        if iv is None:
            out.append(None)
            continue
        if not isinstance(iv, (tuple, list)) or len(iv) != 2 or not all(isinstance(x, numbers.Number) for x in iv):
            raise ValueError(f"guidance_interval[{b}] = {iv!r}: expected (lo, hi)")
        lo, hi = float(iv[0]), float(iv[1])
        if not (lo <= hi):
            raise ValueError(f"guidance_interval[{b}] = ({lo}, {hi}): expected lo <= hi")
        out.append((lo, hi))
    return out


@dataclass
class DiffusionGenerator:
    model: Denoiser
    vae: Any                      # object with .decode(latents) -> (image_tensor, ...); may be None
    device: torch.device
    model_dtype: torch.dtype = torch.float32

    @torch.no_grad()
    def generate(
        self,
        labels: Tensor,
        n_iter: int = 30,
        num_imgs: int = 16,
        class_guidance: float = 3,
        seed: int = 10,
        scale_factor: int = 8,
        img_size: int = 32,
        sharp_f: float = 0.1,
        bright_f: float = 0.1,
        exponent: float = 1,
        seeds: Optional[Tensor] = None,
        noise_levels=None,
        use_ddpm_plus: bool = True,
        guidance_interval=None,
        eta: float = 0.0,
        noise_seeds=None,
        guidance_rescale: float = 0.0,
        apg_eta: float = 1.0,
        apg_norm: float = 0.0,
        apg_momentum: float = 0.0,
    ):
        """Reverse diffusion with classifier-free guidance; returns (decoded_images_on_cpu, latents).

        ``use_ddpm_plus=True``: DPM-Solver++(2M); else DDIM with alpha = 1 - sigma (diffusion.py:45-48).
        ``guidance_interval``, ``eta``, ``noise_seeds``, ``guidance_rescale`` and ``apg_*`` (not in the reference): see ``generate_latents``.
        """
        return self._decode(self.generate_latents(labels, n_iter, num_imgs, class_guidance, seed, img_size, sharp_f, bright_f, exponent,
                                                  seeds, noise_levels, use_ddpm_plus, guidance_interval=guidance_interval, eta=eta,
                                                  noise_seeds=noise_seeds, guidance_rescale=guidance_rescale, apg_eta=apg_eta, apg_norm=apg_norm, apg_momentum=apg_momentum), scale_factor)

    def _decode(self, latents, scale_factor):
        """The exit edge of the three ``generate*`` (diffusion.py:91): (decoded_images_on_cpu, latents); (None, latents) without a VAE."""
        if self.vae is None:
            return None, latents
        return self.vae.decode((latents * scale_factor).to(self.model_dtype))[0].cpu(), latents

    def _in_model_dtype(self, out, trace):
        """The sampler's fp32 latents in ``model_dtype``; with ``trace`` they come with the two fp32 trace tensors, which stay."""
        if trace:
            lat, tx0, txt = out
            return lat.to(self.model_dtype), tx0, txt
        return out.to(self.model_dtype)

    @staticmethod
    def _trajectory(n_iter, exponent, noise_levels, strength, use_ddpm_plus):
        """One request's schedule as the sampler takes it: ``(coeffs, start_mix)``.  ``strength`` None: the whole schedule from pure noise;
        else ``schedule.truncate_levels`` picks the entry level, and ``start_mix`` is that level in float32 (1.0 where nothing was cut:
        pure noise at the first level, as the reference feeds it, diffusion.py:52,59).  Every ``generate_latents*`` builds its scalars
        here, which is what makes a request of a batched call equal its solo call."""
        levels = schedule.noise_schedule(n_iter, exponent, noise_levels)
        k = 0
        if strength is not None:
            k, levels = schedule.truncate_levels(levels, strength)
        return schedule.step_coefficients(levels, use_ddpm_plus), float(np.float32(levels[0])) if k > 0 else 1.0

    @classmethod
    def _trajectory_noise(cls, n_iter, exponent, noise_levels, strength, use_ddpm_plus, eta):
        """``_trajectory`` of a request of the stochastic sampler: ``(coeffs, start_mix, e)`` with ``e`` the float32 noise coefficient per forward
        (``schedule.step_coefficients(levels, use_ddpm_plus, eta)``).  ``eta`` 0 is ``_trajectory`` itself with zeros."""
        if not eta > 0.0:
            coeffs, mix = cls._trajectory(n_iter, exponent, noise_levels, strength, use_ddpm_plus)
            return coeffs, mix, np.zeros(coeffs.shape[0], dtype=np.float32)
        levels = schedule.noise_schedule(n_iter, exponent, noise_levels)
        k = 0
        if strength is not None:
            k, levels = schedule.truncate_levels(levels, strength)
        coeffs, e = schedule.step_coefficients(levels, use_ddpm_plus, eta)
        return coeffs, float(np.float32(levels[0])) if k > 0 else 1.0, e

    @staticmethod
    def _noise_keys(seeds, noise_seeds, num_imgs, seed):
        """The 64-bit noise keys of ``num_imgs`` requests of the stochastic sampler: ``noise_seeds`` (one int each) where given, else
        ``schedule.noise_key`` of the seed that drew each request's start noise and the image's place in that draw -- ``(seed, b)`` under
        one batch seed, ``(seeds[b], 0)`` with one int seed per request.  Start noise handed over as a tensor has no seed: ValueError."""
        if noise_seeds is not None:
            keys = [int(v) & 0xFFFFFFFFFFFFFFFF for v in (noise_seeds.tolist() if isinstance(noise_seeds, Tensor) else noise_seeds)]
            if len(keys) != num_imgs:
                raise ValueError(f"noise_seeds: {len(keys)} entries for {num_imgs} requests")
            return keys
        if seeds is None:
            return [schedule.noise_key(seed, b) for b in range(num_imgs)]
        if isinstance(seeds, Tensor):
            raise ValueError("eta > 0 with the start noise given as a tensor needs noise_seeds (one int per image): a tensor carries no seed to "
                             "derive the noise keys from")
        return [schedule.noise_key(v, 0) for v in seeds]

    @torch.no_grad()
    def generate_latents(self, labels, n_iter=30, num_imgs=16, class_guidance=3, seed=10, img_size=32,
                         sharp_f=0.1, bright_f=0.1, exponent=1, seeds=None, noise_levels=None,
                         use_ddpm_plus=True, trace=False, guidance_interval=None, eta=0.0, noise_seeds=None, guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        """``guidance_interval = (lo, hi)``: limited-interval guidance -- ``class_guidance`` only at the forwards whose noise level lies in
        [lo, hi], the plain conditional prediction elsewhere, where no unconditional sample is run.  The call is then
        ``generate_latents_requests`` with B equal requests; None keeps the path of the reference's sampler untouched.
        ``eta > 0``: the stochastic sampler -- SDE DPM-Solver++(2M), or with ``use_ddpm_plus=False`` DDIM with that eta
        (1: the first-order SDE solver) -- through ``generate_latents_requests`` too; the noise of image b comes from the key
        ``schedule.noise_key(seed, b)``, or ``noise_seeds[b]`` (required when ``seeds`` is a tensor).  0 is the deterministic path, untouched.
        ``guidance_rescale`` (phi in [0, 1]; Lin et al. 2023) and ``apg_eta`` / ``apg_norm`` / ``apg_momentum`` (adaptive projected guidance, Sadat
        et al. 2024: the weight of the update's part parallel to the conditional prediction, the norm the update is clipped to, the momentum over
        the updates) shape the guidance update on the device (``schedule.check_guidance_shape``).  The statistics run over
        each image's whole latent, a masked-out known region included.  Any value other than the defaults takes ``generate_latents_requests``
        too; the defaults are plain CFG on the old path, untouched."""
        eta = schedule.check_eta(eta)
        shape = dict(zip(("apg_eta", "apg_norm", "apg_momentum", "guidance_rescale"),
                         schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)))
        if schedule.guidance_shape_neutral(shape.values()):
            shape = {}
        keys = self._noise_keys(seeds, noise_seeds, num_imgs if seeds is None else len(seeds), seed) if eta > 0.0 else None
        coeffs, _ = self._trajectory(n_iter, exponent, noise_levels, None, use_ddpm_plus)
        x_t = self.initialize_image(seeds, num_imgs, img_size, seed)
        if labels.size(0) != x_t.size(0):
            # the reference zips labels and noise by torch.cat (diffusion.py:61,98)
            raise RuntimeError(f"labels batch {labels.size(0)} != num_imgs {x_t.size(0)}")
        if guidance_interval is not None or keys is not None or shape:
            sde = {} if keys is None else dict(eta=eta, noise_seeds=keys)
            return self.generate_latents_requests(labels, n_iter=n_iter, class_guidance=class_guidance, seeds=x_t, img_size=img_size, sharp_f=sharp_f,
                                                  bright_f=bright_f, exponent=exponent, noise_levels=noise_levels, use_ddpm_plus=use_ddpm_plus,
                                                  trace=trace, guidance_interval=guidance_interval, **sde, **shape)
        self.model.eval()
        return self._in_model_dtype(self.model.sample_latents(x_t, labels.to(self.device), coeffs, class_guidance, sharp_f, bright_f,
                                                              trace=trace), trace)

    @torch.no_grad()
    def generate_from(self, init_latents: Tensor, labels: Tensor, strength: float = 0.6, mask: Optional[Tensor] = None, n_iter: int = 30,
                      num_imgs: Optional[int] = None, class_guidance: float = 3, seed: int = 10, scale_factor: int = 8,
                      img_size: Optional[int] = None, sharp_f: float = 0.1, bright_f: float = 0.1, exponent: float = 1,
                      seeds: Optional[Tensor] = None, noise_levels=None, use_ddpm_plus: bool = True, eta: float = 0.0, noise_seeds=None,
                      guidance_rescale: float = 0.0, apg_eta: float = 1.0, apg_norm: float = 0.0, apg_momentum: float = 0.0):
        """``generate`` for image-to-image and inpainting (``generate_latents_from``); returns (decoded_images_on_cpu, latents)."""
        return self._decode(self.generate_latents_from(init_latents, labels, strength, mask, n_iter, num_imgs, class_guidance, seed, img_size,
                                                       sharp_f, bright_f, exponent, seeds, noise_levels, use_ddpm_plus, eta=eta,
                                                       noise_seeds=noise_seeds, guidance_rescale=guidance_rescale, apg_eta=apg_eta, apg_norm=apg_norm, apg_momentum=apg_momentum), scale_factor)

    @torch.no_grad()
    def generate_latents_from(self, init_latents, labels, strength=0.6, mask=None, n_iter=30, num_imgs=None, class_guidance=3, seed=10,
                              img_size=None, sharp_f=0.1, bright_f=0.1, exponent=1, seeds=None, noise_levels=None, use_ddpm_plus=True,
                              trace=False, guidance_interval=None, eta=0.0, noise_seeds=None, guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        """Reverse diffusion that starts from ``init_latents`` [B,C,S,S] (model space: VAE latent / scale_factor, tld/train.py:122)
        instead of pure noise; the other arguments are ``generate_latents``' (``num_imgs`` / ``img_size`` default to the latents' own).

        ``strength`` in (0, 1] picks the entry point of the schedule (``schedule.truncate_levels``): the latents are noised to the first
        level ``<= strength`` with the training loop's forward process, ``s * eps + (1 - s) * z0`` (tld/train.py:130), ``eps`` being the
        noise ``generate_latents`` would start from for the same ``seed`` / ``seeds``; 1.0 is the text-to-image trajectory, bit for bit.
        ``mask`` [B,1,S,S] in [0,1] at latent resolution (1 = regenerate, 0 = keep): after every step the kept region is set to the same
        forward process of ``init_latents`` at that step's level, and to ``init_latents`` itself in the final prediction (exactly, where
        the mask is 0).  Shapes and ranges are checked on the host before anything is enqueued.  ``guidance_interval = (lo, hi)``: as in
        ``generate_latents``, through ``generate_latents_requests`` with B equal requests; so are ``eta`` and ``noise_seeds`` (with a mask the
        noise is added before the blend: the kept region still rides the forward process of the start noise), and ``guidance_rescale`` and the
        ``apg_*`` controls (their statistics run over the whole latent, the kept region included)."""
        eta = schedule.check_eta(eta)
        shape = dict(zip(("apg_eta", "apg_norm", "apg_momentum", "guidance_rescale"),
                         schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)))
        if schedule.guidance_shape_neutral(shape.values()):
            shape = {}
        if init_latents.dim() != 4:
            raise ValueError(f"init_latents {tuple(init_latents.shape)}: expected [B,C,S,S]")
        B, S = init_latents.shape[0], init_latents.shape[-1]
        num_imgs = B if num_imgs is None else num_imgs
        img_size = S if img_size is None else img_size
        want = (num_imgs, self.model.n_channels, img_size, img_size) if seeds is None else tuple(seeds.shape)
        if tuple(init_latents.shape) != want:
            raise ValueError(f"init_latents {tuple(init_latents.shape)} do not match the noise {want}")
        if labels.size(0) != B:
            raise ValueError(f"labels batch {labels.size(0)} != init_latents batch {B}")
        if mask is not None:
            if tuple(mask.shape) != (B, 1, img_size, img_size):
                raise ValueError(f"mask {tuple(mask.shape)}: expected {(B, 1, img_size, img_size)} (latent resolution; see latent_mask)")
            check_mask_range(mask, " (1 = regenerate, 0 = keep)")
        coeffs, start_mix = self._trajectory(n_iter, exponent, noise_levels, strength, use_ddpm_plus)
        keys = self._noise_keys(seeds, noise_seeds, B, seed) if eta > 0.0 else None
        eps = self.initialize_image(seeds, num_imgs, img_size, seed)
        if guidance_interval is not None or keys is not None or shape:
            sde = {} if keys is None else dict(eta=eta, noise_seeds=keys)
            return self.generate_latents_requests(labels, n_iter=n_iter, class_guidance=class_guidance, seeds=eps, img_size=img_size, sharp_f=sharp_f,
                                                  bright_f=bright_f, exponent=exponent, noise_levels=noise_levels, use_ddpm_plus=use_ddpm_plus,
                                                  init_latents=init_latents, strength=strength, mask=mask, trace=trace,
                                                  guidance_interval=guidance_interval, **sde, **shape)
        self.model.eval()
        return self._in_model_dtype(self.model.sample_latents_from(
            eps, init_latents.to(self.device), labels.to(self.device), coeffs, class_guidance, start_mix,
            mask=None if mask is None else mask.to(self.device), sharp_f=sharp_f, bright_f=bright_f, trace=trace), trace)

    @torch.no_grad()
    def generate_latents_requests(self, labels, *, n_iter=30, class_guidance=3, negative_labels=None, seed=10, seeds=None, img_size=None,
                                  sharp_f=0.1, bright_f=0.1, exponent=1, noise_levels=None, use_ddpm_plus=True, init_latents=None,
                                  strength=None, mask=None, trace=False, guidance_interval=None, guidance_schedule=None, eta=0.0,
                                  noise_seeds=None, guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        """B independent requests in ONE sampler call (``Denoiser.sample_latents_requests``): each of ``n_iter``,
        ``class_guidance``, ``exponent``, ``strength`` and ``use_ddpm_plus`` is a scalar (for all) or a length-B sequence.  Request b's latent
        is bit for bit what ``generate_latents`` / ``generate_latents_from`` return for that request alone with the same noise.

        ``negative_labels``: None, a [B,text] tensor, or a length-B sequence of [text] tensors / None -- the label of the unconditional half
        of the guidance pair instead of zeros (a negative prompt's embedding).  ``seeds``: the noise [B,C,S,S], or one int per request
        (each request's own ``initialize_image(None, 1, size, seed)``, as ``generate_images_from_texts`` draws it); else ``seed`` draws the
        whole batch as ``generate_latents`` does.  ``init_latents`` [B,C,S,S] with ``strength`` (an entry None or 1.0: the text-to-image
        trajectory) and ``mask`` [B,1,S,S] as in ``generate_latents_from``; a sequence entry None stands for zeros (init) / all ones (mask).
        Each request's schedule comes from ``_trajectory``, the function the solo calls use, so its float64 scalars are exactly theirs.
        ``guidance_interval``: ``(lo, hi)`` for all, or one pair / None per request -- the request is guided at ``class_guidance`` only at the
        forwards whose noise level lies in [lo, hi] (``schedule.guidance_table``).  ``guidance_schedule``: one array per request (or None),
        its guidance per forward, one value per level it runs; it wins over the interval and the scalar.  With either, the call is
        ``sample_latents_requests(..., guidance_steps=...)``: a forward whose guidance is exactly 1.0 runs no unconditional sample (DESIGN.md
        section 7.8).
        ``eta``: a scalar or one value per request, 0 where a request stays deterministic.  With any ``eta > 0`` the call is
        ``sample_latents_requests(..., noise_coeffs=..., noise_keys=...)``: request b takes the stochastic solver of its
        own eta, and its noise comes from the key ``noise_seeds[b]`` -- by default ``schedule.noise_key`` of the seed that drew its start noise
        (``(seed, b)``, or ``(seeds[b], 0)`` with one int seed per request; ``seeds`` as a tensor needs ``noise_seeds``).  Request b still equals
        the request alone with the same noise and key, bit for bit.
        ``guidance_rescale``, ``apg_eta``, ``apg_norm``, ``apg_momentum``: each a scalar or one value per request (``generate_latents``;
        DESIGN.md section 7.16).  With any value other than the defaults the call is ``sample_latents_requests(..., shape=...)``; a request at
        the defaults runs plain CFG inside it, and request b still equals the request alone, bit for bit.
        Shapes and ranges are checked on the host before anything is enqueued."""
        B = labels.size(0)
        size = self.model.image_size if img_size is None else img_size

        def per_request(v, what):
            if isinstance(v, (numbers.Number, bool, type(None))) or (isinstance(v, Tensor) and v.dim() == 0):
                return [v] * B
            v = list(v)
            if len(v) != B:
                raise ValueError(f"{what}: {len(v)} entries for {B} requests")
            return v

        n_it, guid = per_request(n_iter, "n_iter"), per_request(class_guidance, "class_guidance")
        expo, plus, stren = per_request(exponent, "exponent"), per_request(use_ddpm_plus, "use_ddpm_plus"), per_request(strength, "strength")
        etas = [schedule.check_eta(v) for v in per_request(eta, "eta")]
        keys = self._noise_keys(seeds, noise_seeds, B, seed) if any(v > 0.0 for v in etas) else None
        shape_rows = schedule.guidance_shape_rows(B, guidance_rescale, apg_eta, apg_norm, apg_momentum)
        for b in range(B):
            if not np.isfinite(float(guid[b])):
                raise ValueError(f"class_guidance[{b}] = {guid[b]} is not finite")
        z0 = stack_optional(init_latents, "init_latents", B, (self.model.n_channels, size, size), 0.0)
        m = stack_optional(mask, "mask", B, (1, size, size), 1.0)
        if m is not None:
            check_mask_range(m, " (1 = regenerate, 0 = keep)")
        if z0 is None and (m is not None or any(v is not None and float(v) != 1.0 for v in stren)):
            raise ValueError("init_latents is required with a mask or a strength below 1")
        coeffs, mix, ecs = [], [], []
        for b in range(B):
            if int(n_it[b]) < 2 and noise_levels is None:
                raise ValueError(f"n_iter[{b}] = {n_it[b]}: a trajectory needs at least two noise levels")
            if keys is None:
                co, s0 = self._trajectory(int(n_it[b]), expo[b], noise_levels, stren[b], bool(plus[b]))
            else:
                co, s0, e = self._trajectory_noise(int(n_it[b]), expo[b], noise_levels, stren[b], bool(plus[b]), etas[b])
                ecs.append(e)
            coeffs.append(co)
            mix.append(s0)
        steps = None
        if guidance_interval is not None or guidance_schedule is not None:
            ivs = per_request_intervals(guidance_interval, B)
            sched = [None] * B if guidance_schedule is None else list(guidance_schedule)
            if len(sched) != B:
                raise ValueError(f"guidance_schedule: {len(sched)} entries for {B} requests")
            steps = []
            for b in range(B):
                if sched[b] is None:
                    steps.append(schedule.guidance_table(coeffs[b], float(guid[b]), ivs[b]))
                    continue
                t = np.ascontiguousarray(torch.as_tensor(sched[b]).detach().cpu().numpy() if isinstance(sched[b], Tensor) else sched[b], dtype=np.float32)
                if t.ndim != 1 or t.shape[0] != coeffs[b].shape[0]:
                    raise ValueError(f"guidance_schedule[{b}] {t.shape}: expected [{coeffs[b].shape[0]}], one value per forward")
                if not np.isfinite(t).all():
                    raise ValueError(f"guidance_schedule[{b}] holds a value that is not finite")
                steps.append(t)
        eps = self._noise(seeds, B, size, seed)
        if eps.size(0) != B:
            raise RuntimeError(f"labels batch {B} != noise batch {eps.size(0)}")
        self.model.eval()
        kw = {} if steps is None else dict(guidance_steps=steps)
        if keys is not None:
            kw.update(noise_coeffs=ecs, noise_keys=keys)
        if shape_rows is not None:
            kw.update(shape=shape_rows)
        return self._in_model_dtype(self.model.sample_latents_requests(
            eps, labels.to(self.device), coeffs, [float(g) for g in guid], neg_labels=negative_labels, init_latents=z0, start_mix=mix,
            mask=m, sharp_f=sharp_f, bright_f=bright_f, trace=trace, **kw), trace)

    @torch.no_grad()
    def generate_requests(self, labels, *, scale_factor: int = 8, **kw):
        """``generate_latents_requests`` plus the VAE decode; returns (decoded_images_on_cpu, latents)."""
        kw.pop("trace", None)
        return self._decode(self.generate_latents_requests(labels, **kw), scale_factor)

    def open_session(self, slots: int, img_size: Optional[int] = None, sharp_f: float = 0.1, bright_f: float = 0.1, cond_rows: Optional[int] = None) -> "SamplerSession":
        """A sampler session: up to ``slots`` requests run at once, each at its own level; ``SamplerSession.admit`` puts a
        request in between steps, ``step`` runs one model forward for every live request, and a request leaves at its final forward with, bit for
        bit, the latent ``generate_latents_requests`` returns for it alone.  ``sharp_f`` / ``bright_f`` are per session.  Use it as a context manager."""
        size = self.model.image_size if img_size is None else int(img_size)
        if size != self.model.image_size:
            raise ValueError(f"img_size {size}: a session runs at the model's own size {self.model.image_size}")
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            raise ValueError("sharded sampling is not part of a sampler session: open one session per rank's own requests")
        self.model.eval()
        return SamplerSession(self, self.model.open_session(slots, cond_rows, sharp_f, bright_f, device=self.device))

    def _noise(self, seeds, num_imgs, img_size, seed):
        """``initialize_image`` where ``seeds`` may also be one int per image: image i then starts from its own
        ``initialize_image(None, 1, img_size, seeds[i])``, the noise of a one-image call with that seed."""
        if seeds is None or isinstance(seeds, Tensor):
            return self.initialize_image(seeds, num_imgs, img_size, seed)
        seeds = list(seeds)
        if len(seeds) != num_imgs:
            raise ValueError(f"seeds: {len(seeds)} entries for {num_imgs} requests")
        if not seeds:
            return self.initialize_image(None, 0, img_size, seed)
        return torch.cat([self.initialize_image(None, 1, img_size, int(v)) for v in seeds])

    def initialize_image(self, seeds, num_imgs, img_size, seed):
        """Initial noise (diffusion.py:105-120): the caller's ``seeds`` tensor, or ``torch.randn`` from a
        generator seeded with ``seed``.

        The generator lives on the HOST (``torch.Generator('cpu')``), whatever ``self.device`` is: parity is
        stated against the reference's CPU path, whose generator is the CPU one (``device`` = cpu there), so
        ``seed=`` reproduces the reference's x_T bit for bit (tests/golden g2 ``seed10_xT``); it also makes the
        noise independent of the number of ranks a batch is later sharded over.  The draw is one small tensor
        per call, moved to the device once."""
        if seeds is None:
            generator = torch.Generator(device="cpu")
            generator.manual_seed(seed)
            x = torch.randn(num_imgs, self.model.n_channels, img_size, img_size, dtype=self.model_dtype,
                            generator=generator)
            return x.to(self.device)
        return seeds.to(self.device, self.model_dtype)


def download_file(url, filename):
    import requests
    with requests.get(url, stream=True) as r:
        r.raise_for_status()
        with open(filename, "wb") as f:
            for chunk in r.iter_content(chunk_size=8192):
                f.write(chunk)


def make_image_grid(images: Tensor, nrow: int, padding: int = 4) -> Tensor:
    """[B,C,H,W] -> [C, rows*(H+pad)+pad, cols*(W+pad)+pad] grid with zero padding (the layout the
    reference obtains from torchvision.utils.make_grid at diffusion.py:185)."""
    b, c, h, w = images.shape
    if b == 1:
        return images[0]
    cols = min(nrow, b)
    rows = (b + cols - 1) // cols
    grid = images.new_zeros((c, rows * (h + padding) + padding, cols * (w + padding) + padding))
    for k in range(b):
        r, q = divmod(k, cols)
        y0, x0 = r * (h + padding) + padding, q * (w + padding) + padding
        grid[:, y0:y0 + h, x0:x0 + w] = images[k]
    return grid


def latent_mask(mask, latent_size: int) -> Tensor:
    """Pixel-resolution inpainting mask -> latent resolution by area averaging: a PIL "L" image (0..255) or a tensor [H,W] / [1,H,W] in
    [0,1], square, with H a multiple of ``latent_size``; returns fp32 [1, latent_size, latent_size] in [0,1] (1 = regenerate).  A latent
    cell is kept exactly (0) only where every pixel under it is 0."""
    if not isinstance(mask, Tensor):
        arr = np.array(mask.convert("L") if hasattr(mask, "convert") else mask)
        mask = torch.from_numpy(arr).to(torch.float32) / (255.0 if arr.dtype == np.uint8 else 1.0)
    m = mask.detach().to(torch.float32)
    if m.dim() == 3 and m.shape[0] == 1:
        m = m[0]
    if m.dim() != 2 or m.shape[0] != m.shape[1]:
        raise ValueError(f"mask {tuple(mask.shape)}: expected a square [H,W] or [1,H,W]")
    H = m.shape[0]
    if latent_size <= 0 or H % latent_size:
        raise ValueError(f"mask side {H} is not a multiple of the latent size {latent_size}")
    check_mask_range(m)
    f = H // latent_size
    return m.reshape(latent_size, f, latent_size, f).mean(dim=(1, 3)).clamp_(0.0, 1.0).unsqueeze(0)


def to_pil(img: Tensor):
    from PIL import Image
    arr = (img.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).cpu().numpy()
    return Image.fromarray(arr.squeeze(-1) if arr.shape[-1] == 1 else arr)


class DiffusionTransformer:
    """Text -> image pipeline shell (diffusion.py:143-186).

    ``vae`` / ``clip_model`` / ``text_encoder`` may be injected; otherwise ``diffusers`` and ``clip`` are
    imported lazily exactly where the reference uses them and a missing package raises ImportError.
    ``tokenizer``: a ``ClipTokenizer`` (clip_tokenizer.py) or the path of CLIP's merges file -- prompts are then tokenised here
    (``clip.tokenize(prompts, truncate=True)``, diffusion.py:136) and, with ``clip_model=ClipTextEncoder(...)``, the whole
    text -> label edge runs without the ``clip`` package.
    ``low_latency``: serve small batches in one of the denoiser's low-latency capacity classes (``Denoiser.set_low_latency``): ``True`` / ``1`` = up to 4096
    token rows per sampler call (8 images at 256 px), ``2`` = up to 1024 (one or two images: one prompt per call) -- a one-image 35-step ``generate`` takes 31 /
    30 ms instead of 37; larger batches then raise (use a second pipeline object for bulk work).
    """

    def __init__(self, cfg: LTDConfig, vae: Any = None, clip_model: Any = None, text_encoder=None,
                 run_device: Optional[torch.device] = None, tokenizer: Any = None, low_latency=False):
        dev = run_device if run_device is not None else device
        denoiser = Denoiser(**asdict(cfg.denoiser_cfg))
        denoiser = denoiser.to(cfg.denoiser_load.dtype)
        if low_latency:      # one-prompt-per-call serving (tld/app.py:48-65): the denoiser's small-batch capacity class (Denoiser.set_low_latency)
            denoiser.set_low_latency(low_latency)
        if cfg.denoiser_load.file_url is not None and cfg.denoiser_load.local_filename is not None:
            print(f"Downloading model from {cfg.denoiser_load.file_url}")
            download_file(cfg.denoiser_load.file_url, cfg.denoiser_load.local_filename)
            state_dict = torch.load(cfg.denoiser_load.local_filename, map_location=torch.device("cpu"))
            denoiser.load_state_dict(state_dict)
        denoiser = denoiser.to(dev)
        if vae is None:
            from diffusers import AutoencoderKL   # third-party exit edge
            vae = AutoencoderKL.from_pretrained(cfg.vae_cfg.vae_name, torch_dtype=cfg.vae_cfg.vae_dtype).to(dev)
        self._text_encoder = text_encoder
        if isinstance(tokenizer, (str, os.PathLike)):
            from .clip_tokenizer import ClipTokenizer
            tokenizer = ClipTokenizer(bpe_path=tokenizer)
        self._tokenizer = tokenizer
        if clip_model is None and text_encoder is None:
            import clip                            # third-party entry edge
            clip_model, _ = clip.load(cfg.clip_cfg.clip_model_name)
            clip_model = clip_model.to(dev)
        self.clip_model = clip_model
        self.device = dev
        self.diffuser = DiffusionGenerator(denoiser, vae, dev, cfg.denoiser_load.dtype)

    def tokenize(self, prompts) -> Tensor:
        if self._tokenizer is not None:
            return self._tokenizer.tokenize(prompts, truncate=True)
        import clip
        return clip.tokenize(prompts, truncate=True)

    def _labels(self, texts) -> Tensor:
        """The text encoder's labels of ``texts``, on the device it leaves them on: the injected ``text_encoder``, else CLIP over ``tokenize``."""
        if self._text_encoder is not None:
            return self._text_encoder(texts)
        return self.clip_model.encode_text(self.tokenize(texts).to(self.device))

    @torch.no_grad()
    def encode_text(self, prompts):
        return self._labels(prompts).cpu()

    @torch.no_grad()
    def clip_scores(self, images, prompts) -> Tensor:
        """CLIP score of each picture against its prompt: cosine of ``clip_model.encode_image(clip_preprocess(images))`` with the prompt's label.
        ``images``: PIL images or a float tensor ``[B, 3, H, W]`` in [0, 1]; ``prompts``: one string per image.  Returns ``[B]`` fp32 on the device.
        Needs a ``clip_model`` with an image tower (``Clip(text, visual)`` or what ``clip.load`` returns)."""
        from .clip_image import clip_preprocess, clip_score
        if self.clip_model is None or not hasattr(self.clip_model, "encode_image"):
            raise RuntimeError("clip_scores needs a clip_model with encode_image (the image tower): pass clip_model=Clip(text=..., visual=...); "
                               f"this pipeline holds {type(self.clip_model).__name__}")
        prompts = [prompts] if isinstance(prompts, str) else list(prompts)
        pixels = clip_preprocess(images, self.clip_model.visual.input_resolution).to(self.device)
        if pixels.shape[0] != len(prompts):
            raise ValueError(f"clip_scores: {pixels.shape[0]} images but {len(prompts)} prompts")
        return clip_score(self.clip_model.encode_image(pixels).float(), self._labels(prompts).to(self.device).float())

    @torch.no_grad()
    def image_features(self, images, bank=None) -> Tensor:
        """CLIP image embeddings of arbitrary pictures, ``clip_model.encode_image(clip_preprocess(images))``: PIL images or a float tensor
        ``[B, 3, H, W]`` in [0, 1] -> ``[B, embed_dim]`` fp32 on the device; with ``bank`` (a ``metrics.FeatureBank``) they are appended to it as
        well.  This builds the reference bank of real images that ``metrics.cmmd`` / ``metrics.frechet_distance`` compare generated samples with
        (``Trainer.eval_features`` fills the other one).  Needs a ``clip_model`` with an image tower, like ``clip_scores``."""
        from .metrics import image_embeddings
        if self.clip_model is None or not hasattr(self.clip_model, "encode_image"):
            raise RuntimeError("image_features needs a clip_model with encode_image (the image tower): pass clip_model=Clip(text=..., visual=...); "
                               f"this pipeline holds {type(self.clip_model).__name__}")
        emb = image_embeddings(self.clip_model, images, self.device)
        if bank is not None:
            bank.add(emb)
        return emb

    @torch.no_grad()
    def generate_images_from_texts(self, prompts, class_guidance=6, seeds=11, n_iter=15, negative_prompts=None, guidance_interval=None, eta=0.0,
                                   guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        """Batched front edge (the reference serves one prompt per call, tld/app.py:48-65):
        one text-encoder call for all prompts, labels stay on the device, ONE sampler call (sample-sharded over the
        ranks of the default process group when torch.distributed is initialised), one VAE decode; returns one PIL image
        per prompt.  ``seeds``: an int (request i uses seeds + i) or one int per prompt.  Request i's picture is exactly
        what ``generate_image_from_text(prompts[i], seed=seeds[i])`` returns: samples never interact.
        ``class_guidance`` / ``n_iter`` may be one value per prompt and ``negative_prompts`` one string (or None) per prompt, or one string
        for all: the sampler call is then ``generate_latents_requests`` (still one call), and a negative
        prompt is encoded with the same text encoder in the same call as the prompts.  Scalars and no negatives call ``generate_latents``;
        the seeds and noise before the sampler call and the decode and pictures after it are the same code for both.
        ``guidance_interval``: ``(lo, hi)`` for all prompts or one pair / None per prompt -- limited-interval guidance
        (``generate_latents_requests``); the call is then the requests one.
        ``eta``: one value or one per prompt; any ``eta > 0`` makes it the requests call with the stochastic sampler.
        Request i's noise key is ``schedule.noise_key(seeds[i])``, that of the one-prompt call with its seed, so the pictures still agree.
        ``guidance_rescale``, ``apg_eta``, ``apg_norm``, ``apg_momentum``: one value or one per prompt (``DiffusionGenerator.generate_latents``,
        DESIGN.md section 7.16); any value other than the defaults makes it the requests call."""
        from .sharded import sharded_sample
        prompts = list(prompts)
        n = len(prompts)
        if n == 0:
            return []
        seed_list = [int(seeds) + i for i in range(n)] if isinstance(seeds, numbers.Integral) else [int(v) for v in seeds]
        if len(seed_list) != n:
            raise ValueError(f"{len(seed_list)} seeds for {n} prompts")
        gen, size = self.diffuser, self.diffuser.model.image_size
        etas = [schedule.check_eta(v) for v in ([eta] * n if isinstance(eta, numbers.Number) else list(eta))]
        if len(etas) != n:
            raise ValueError(f"{len(etas)} eta values for {n} prompts")
        noisy = any(v > 0.0 for v in etas)
        shape_rows = schedule.guidance_shape_rows(n, guidance_rescale, apg_eta, apg_norm, apg_momentum)     # (eta_par, norm_r, beta, phi) per prompt, or None
        if (isinstance(class_guidance, numbers.Number) and isinstance(n_iter, numbers.Number) and negative_prompts is None and guidance_interval is None
                and not noisy and shape_rows is None):
            labels, extras = self._labels(prompts).to(self.device, torch.float32), ()

            def one(xs, ls):
                return gen.generate_latents(ls, n_iter=n_iter, num_imgs=xs.shape[0], class_guidance=class_guidance, img_size=size,
                                            sharp_f=0, bright_f=0, exponent=1, seeds=xs)
        else:
            def per_prompt(v, what):
                v = [v] * n if isinstance(v, numbers.Number) else list(v)
                if len(v) != n:
                    raise ValueError(f"{len(v)} {what} values for {n} prompts")
                return v

            guid, n_it = [float(g) for g in per_prompt(class_guidance, "class_guidance")], [int(k) for k in per_prompt(n_iter, "n_iter")]
            labels, neg_rows = self._encode_with_negatives(prompts, negative_prompts)
            extras = (torch.arange(n),)
            ivs = None if guidance_interval is None else per_request_intervals(guidance_interval, n)

            def one(xs, ls, which):           # the per-request scalars ride as the requests' indices, sliced like every per-sample tensor
                w = [int(i) for i in which]
                kw = {} if ivs is None else dict(guidance_interval=[ivs[i] for i in w])
                if noisy:
                    kw.update(eta=[etas[i] for i in w], noise_seeds=[schedule.noise_key(seed_list[i]) for i in w])
                if shape_rows is not None:
                    kw.update(apg_eta=[shape_rows[i][0] for i in w], apg_norm=[shape_rows[i][1] for i in w],
                              apg_momentum=[shape_rows[i][2] for i in w], guidance_rescale=[shape_rows[i][3] for i in w])
                return gen.generate_latents_requests(ls, n_iter=[n_it[i] for i in w], class_guidance=[guid[i] for i in w],
                                                     negative_labels=None if neg_rows is None else [neg_rows[i] for i in w], seeds=xs, img_size=size,
                                                     sharp_f=0, bright_f=0, exponent=1, **kw)

        x_T = gen._noise(seed_list, n, size, 0)                                          # each request's own noise
        out = gen._decode(sharded_sample(one, x_T, labels, extras=extras), 8)[0]         # scale_factor 8 (diffusion.py:180)
        return [to_pil(((out[i] + 1) / 2).float().clip(0, 1)) for i in range(n)]

    def _encode_with_negatives(self, prompts, negative_prompts):
        """Labels of ``prompts`` and of the negative prompts that are not None, from ONE text-encoder call: (labels [n,text], list of n
        [text] rows / None, or None when no request has a negative prompt)."""
        n = len(prompts)
        if negative_prompts is None or isinstance(negative_prompts, str):
            negs = [negative_prompts] * n
        else:
            negs = list(negative_prompts)
            if len(negs) != n:
                raise ValueError(f"{len(negs)} negative prompts for {n} prompts")
        texts = list(prompts) + [str(p) for p in negs if p is not None]
        emb = self._labels(texts).to(self.device, torch.float32)
        if len(texts) == n:
            return emb, None
        rows, k = [], n
        for p in negs:
            rows.append(None if p is None else emb[k])
            k += p is not None
        return emb[:n], rows

    def generate_image_from_text(self, prompt: str, class_guidance=6, seed=11, num_imgs=1, img_size=32, n_iter=15, *, negative_prompt=None,
                                 guidance_interval=None, eta=0.0, guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        nrow = int(np.sqrt(num_imgs))
        giv = {} if guidance_interval is None else dict(guidance_interval=guidance_interval)      # limited-interval guidance
        if schedule.check_eta(eta) > 0.0:     # the stochastic sampler: image b's noise key is schedule.noise_key(seed, b)
            giv["eta"] = eta
        row = schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)
        if not schedule.guidance_shape_neutral(row):      # guidance rescale / APG
            giv.update(apg_eta=row[0], apg_norm=row[1], apg_momentum=row[2], guidance_rescale=row[3])
        if negative_prompt is not None:       # the unconditional half of the guidance pair reads the negative prompt's label instead of zeros
            labels, neg = self._encode_with_negatives([prompt] * num_imgs, [negative_prompt] + [None] * (num_imgs - 1))
            out, _ = self.diffuser.generate_requests(labels, negative_labels=[neg[0]] * num_imgs, n_iter=n_iter, class_guidance=class_guidance,
                                                     seed=seed, exponent=1, scale_factor=8, sharp_f=0, bright_f=0, **giv)
        elif giv:
            out, _ = self.diffuser.generate_requests(self.encode_text([prompt] * num_imgs), n_iter=n_iter, class_guidance=class_guidance, seed=seed,
                                                     exponent=1, scale_factor=8, sharp_f=0, bright_f=0, **giv)
        else:
            # NOTE: like the reference, ``img_size`` is ignored in favour of the model's own size (:175)
            out, _ = self.diffuser.generate(
                labels=self.encode_text([prompt] * num_imgs), num_imgs=num_imgs, img_size=self.diffuser.model.image_size,
                class_guidance=class_guidance, seed=seed, n_iter=n_iter, exponent=1, scale_factor=8, sharp_f=0,
                bright_f=0)
        return to_pil(make_image_grid((out + 1) / 2, nrow=nrow, padding=4).float().clip(0, 1))

    @torch.no_grad()
    def generate_image_from_image(self, image, prompt: str, strength=0.6, mask=None, class_guidance=6, seed=11, n_iter=15,
                                  sample_posterior=False, return_latents=False, *, negative_prompt=None, guidance_interval=None, eta=0.0,
                                  guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
        """Image -> image: edit ``image`` towards ``prompt`` at ``strength``, or with ``mask`` regenerate only the masked region.

        ``image``: a PIL image or a [3,H,W] tensor in [0,1] with H = W = 8 x the model's latent size (no resizing here).  It is encoded
        with the pipeline's VAE (``vae.encode(2 x - 1).latent_dist``: ``.mode()``, or ``.sample()`` from a generator seeded with ``seed``
        when ``sample_posterior``) and divided by 8 (tld/train.py:122).  ``mask``: PIL "L" image or tensor [H,W] / [1,H,W] at pixel
        resolution, 1 = regenerate; it is area-averaged to the latent grid (``latent_mask``), so only latent cells whose 8 x 8 pixels are
        all 0 are kept exactly.  Sampler settings as in ``generate_image_from_text``; with ``negative_prompt`` the unconditional half of
        the guidance pair reads that prompt's label (``generate_requests``); ``guidance_interval = (lo, hi)`` guides only at the noise levels
        inside it (the same entry); ``eta > 0`` takes the stochastic sampler (the same entry; noise key ``schedule.noise_key(seed)``);
        so do ``guidance_rescale`` and the ``apg_*`` controls (their statistics run over the whole latent, the kept region of
        a mask included).  Returns a PIL image (with ``return_latents``: (image, latents))."""
        gen = self.diffuser
        size = gen.model.image_size
        if not isinstance(image, Tensor):
            if not hasattr(image, "convert"):
                raise ValueError("image: expected a PIL image or a [3,H,W] tensor in [0,1]")
            image = torch.from_numpy(np.asarray(image.convert("RGB")).copy()).permute(2, 0, 1).to(torch.float32) / 255.0
        if image.dim() != 3 or tuple(image.shape) != (3, 8 * size, 8 * size):
            raise ValueError(f"image {tuple(image.shape)}: expected [3, {8 * size}, {8 * size}] (8 x the model's {size} x {size} latents)")
        if image.numel() and not (float(image.min()) >= 0.0 and float(image.max()) <= 1.0):
            raise ValueError("image values outside [0, 1]")
        m = None
        if mask is not None:
            side = mask.size[0] if hasattr(mask, "convert") else mask.shape[-1]
            if side != 8 * size:
                raise ValueError(f"mask side {side}: expected the image's {8 * size}")
            m = latent_mask(mask, size).unsqueeze(0)
        neg = None
        if negative_prompt is None:
            labels = self.encode_text([prompt])
        else:
            labels, neg = self._encode_with_negatives([prompt], [negative_prompt])
        x = (image.to(self.device, torch.float32) * 2 - 1).unsqueeze(0)
        x = x.to(getattr(gen.vae, "dtype", torch.float32))
        dist_ = gen.vae.encode(x).latent_dist
        if sample_posterior:
            z = dist_.sample(generator=torch.Generator(device="cpu").manual_seed(int(seed)))
        else:
            z = dist_.mode()
        z0 = z.to(torch.float32) / 8
        row = schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)
        shaped = not schedule.guidance_shape_neutral(row)
        if neg is not None or guidance_interval is not None or schedule.check_eta(eta) > 0.0 or shaped:
            giv = {} if guidance_interval is None else dict(guidance_interval=guidance_interval)
            if eta > 0.0:
                giv["eta"] = eta
            if shaped:
                giv.update(apg_eta=row[0], apg_norm=row[1], apg_momentum=row[2], guidance_rescale=row[3])
            out, latents = gen.generate_requests(labels, negative_labels=neg, init_latents=z0, strength=strength, mask=m, n_iter=n_iter,
                                                 class_guidance=class_guidance, seed=seed, exponent=1, scale_factor=8, sharp_f=0, bright_f=0, **giv)
        else:
            out, latents = gen.generate_from(z0, labels, strength=strength, mask=m, n_iter=n_iter, class_guidance=class_guidance, seed=seed,
                                             exponent=1, scale_factor=8, sharp_f=0, bright_f=0)
        pic = to_pil(((out[0] + 1) / 2).float().clip(0, 1))
        return (pic, latents) if return_latents else pic

class SamplerSession:
    """A sampler session of a ``DiffusionGenerator`` (``open_session``).  Requests are built by the helpers the
    ``generate_latents*`` calls use (``_trajectory``, ``schedule.guidance_table``, ``schedule.noise_key``), so a request's tables are the solo call's
    tables and its latent the solo call's latent, bit for bit."""

    # what a request of the other sampler entries may bring and a session does not take
    OUT_OF_SCOPE = {"init_latents": "init_latents (image-to-image)", "strength": "strength (start_mix < 1)", "mask": "mask (inpainting)",
                    "guidance_rescale": "guidance_rescale (the guidance shape)", "apg_eta": "apg_eta (the guidance shape)",
                    "apg_norm": "apg_norm (the guidance shape)", "apg_momentum": "apg_momentum (the guidance shape)", "trace": "trace"}

    def __init__(self, generator: "DiffusionGenerator", raw):
        self.generator, self.raw = generator, raw
        self._ticket_of = {}              # slot -> ticket of the request in it
        self._next = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    @torch.no_grad()
    def admit(self, label: Tensor, *, n_iter=30, class_guidance=3, negative_label=None, seed=10, noise=None, exponent=1, use_ddpm_plus=True,
              noise_levels=None, guidance_interval=None, guidance_schedule=None, eta=0.0, noise_seed=None, **other):
        """One request: ``label`` [text] (or [1,text]) and the scalars of ``generate_latents_requests`` for one request.  ``noise``: its start noise
        [C,S,S], else ``initialize_image(None, 1, size, seed)``.  ``eta > 0``: its noise key is ``noise_seed``, else ``schedule.noise_key(seed)``
        (a ``noise`` tensor carries no seed: ``noise_seed`` is then required).  Returns a ticket, or None when the session has no room now."""
        for k in other:
            if k in self.OUT_OF_SCOPE:
                raise ValueError(f"{self.OUT_OF_SCOPE[k]} is not part of a sampler session")
            raise TypeError(f"admit() got an unexpected keyword argument {k!r}")
        gen = self.generator
        eta = schedule.check_eta(eta)
        if not np.isfinite(float(class_guidance)):
            raise ValueError(f"class_guidance = {class_guidance} is not finite")
        if int(n_iter) < 2 and noise_levels is None:
            raise ValueError(f"n_iter = {n_iter}: a trajectory needs at least two noise levels")
        key = ecs = None
        if eta > 0.0:
            if noise_seed is None and noise is not None:
                raise ValueError("eta > 0 with the start noise given as a tensor needs noise_seed: a tensor carries no seed to derive the noise key from")
            key = schedule.noise_key(seed, 0) if noise_seed is None else int(noise_seed) & 0xFFFFFFFFFFFFFFFF
            coeffs, _, ecs = gen._trajectory_noise(int(n_iter), exponent, noise_levels, None, bool(use_ddpm_plus), eta)
        else:
            coeffs, _ = gen._trajectory(int(n_iter), exponent, noise_levels, None, bool(use_ddpm_plus))
        steps = None
        if guidance_schedule is not None:
            steps = np.ascontiguousarray(torch.as_tensor(guidance_schedule).detach().cpu().numpy() if isinstance(guidance_schedule, Tensor) else guidance_schedule,
                                         dtype=np.float32)
            if steps.ndim != 1 or steps.shape[0] != coeffs.shape[0]:
                raise ValueError(f"guidance_schedule {steps.shape}: expected [{coeffs.shape[0]}], one value per forward")
            if not np.isfinite(steps).all():
                raise ValueError("guidance_schedule holds a value that is not finite")
        elif guidance_interval is not None:
            steps = schedule.guidance_table(coeffs, float(class_guidance), per_request_intervals(guidance_interval, 1)[0])
        size = gen.model.image_size
        eps = gen.initialize_image(None, 1, size, int(seed)) if noise is None else noise.to(gen.device, gen.model_dtype)
        slot = self.raw.admit(eps, label.to(gen.device), coeffs, float(class_guidance), neg_label=negative_label, guidance_steps=steps, noise_coeff=ecs,
                              noise_key=key)
        if slot is None:
            return None
        ticket = self._next
        self._next += 1
        self._ticket_of[slot] = ticket
        return ticket

    @torch.no_grad()
    def step(self):
        """One step of every live request; returns ``{ticket: latent [C,S,S]}`` of the requests that finished in it (copies, in ``model_dtype``)."""
        return {self._ticket_of.pop(slot): self.raw.latent(slot).to(self.generator.model_dtype) for slot in self.raw.step()}

    @property
    def live(self) -> int:
        return self.raw.live

    def stats(self) -> dict:
        return self.raw.stats()

    def close(self):
        self.raw.close()


class ContinuousBatcher:
    """Serving-side batching with admission between steps (beside ``RequestBatcher``): one sampler session of ``slots``
    slots over the pipeline's denoiser.  ``submit`` encodes the text and queues the request; ``step`` admits queued requests in submission order
    while the session has room, runs one step and returns ``{ticket: PIL.Image}`` for the requests that finished; ``drain`` steps until nothing is
    queued or live.  A request's picture is what ``generate_images_from_texts`` returns for that prompt alone."""

    def __init__(self, pipeline: "DiffusionTransformer", slots: int = 8):
        self.pipeline = pipeline
        self.session = pipeline.diffuser.open_session(slots, sharp_f=0, bright_f=0)
        self._queue = []                  # (ticket, label, negative label, admit keywords)
        self._ticket_of = {}              # the session's ticket -> ours
        self._next = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def close(self):
        self.session.close()

    @torch.no_grad()
    def submit(self, prompt: str, class_guidance: float = 6, seed: int = 11, n_iter: int = 15, negative_prompt: Optional[str] = None,
               guidance_interval=None, eta: float = 0.0, guidance_rescale: float = 0.0, apg_eta: float = 1.0, apg_norm: float = 0.0,
               apg_momentum: float = 0.0) -> int:
        eta = schedule.check_eta(eta)
        if not schedule.guidance_shape_neutral(schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)):
            raise ValueError("the guidance shape (guidance_rescale / apg_*) is not part of a sampler session: use RequestBatcher(mixed=True)")
        interval = per_request_intervals(guidance_interval, 1)[0] if guidance_interval is not None else None
        if int(n_iter) < 2:
            raise ValueError(f"n_iter = {n_iter}: a trajectory needs at least two noise levels")
        labels, neg = self.pipeline._encode_with_negatives([str(prompt)], None if negative_prompt is None else [str(negative_prompt)])
        kw = dict(n_iter=int(n_iter), class_guidance=float(class_guidance), seed=int(seed), exponent=1, guidance_interval=interval)
        if eta > 0.0:
            kw.update(eta=eta, noise_seed=schedule.noise_key(int(seed)))
        ticket = self._next
        self._next += 1
        self._queue.append((ticket, labels[0], None if neg is None else neg[0], kw))
        return ticket

    def pending(self) -> int:
        return len(self._queue)

    @property
    def live(self) -> int:
        return self.session.live

    @torch.no_grad()
    def step(self):
        while self._queue:
            ticket, label, neg, kw = self._queue[0]
            t = self.session.admit(label, negative_label=neg, **kw)
            if t is None:
                break
            self._ticket_of[t] = ticket
            self._queue.pop(0)
        done = self.session.step()
        if not done:
            return {}
        order = sorted(done)
        out = self.pipeline.diffuser._decode(torch.stack([done[t] for t in order]), 8)[0]      # scale_factor 8 (diffusion.py:180)
        return {self._ticket_of.pop(t): to_pil(((out[i] + 1) / 2).float().clip(0, 1)) for i, t in enumerate(order)}

    def drain(self):
        """Steps until nothing is queued or live; returns every picture of those steps."""
        out = {}
        while self._queue or self.session.live:      # (an empty session takes any request that can fit at all; one that cannot makes admit raise)
            out.update(self.step())
        return out


class _Request(NamedTuple):
    """One queued request of ``RequestBatcher``."""
    ticket: int
    prompt: str
    class_guidance: float
    seed: int
    n_iter: int
    negative_prompt: Optional[str]


class RequestBatcher:
    """Groups text-to-image requests into batched sampler calls (serving-side batching; the reference's FastAPI
    handler runs the blocking pipeline once per request, tld/app.py:48-65).

    ``class_guidance`` and ``n_iter`` are per-call scalars of the sampler, so requests are grouped by that pair;
    inside a group every request keeps its own prompt and seed.  Synchronous by design: ``submit`` queues,
    ``flush`` runs the queued groups (largest first, at most ``max_batch`` requests per sampler call) and returns
    ``{ticket: PIL.Image}``.

    ``mixed=True``: a sampler call carries requests with different scalars (``generate_images_from_texts`` with one guidance value and
    one ``n_iter`` per prompt), so calls are filled in submission order up to ``max_batch`` whatever the scalars
    are, a request may bring a negative prompt, and a new call starts where the conditioning rows of one call (distinct noise levels +
    label rows) would pass ``schedule.REQUEST_ROW_CAP``."""

    def __init__(self, pipeline: "DiffusionTransformer", max_batch: int = 64, mixed: bool = False):
        self.pipeline = pipeline
        self.max_batch = int(max_batch)
        self.mixed = bool(mixed)
        self._queue = []
        self._intervals = {}               # ticket -> (lo, hi) of the requests that brought a guidance interval
        self._etas = {}                    # ticket -> eta of the requests that asked for the stochastic sampler
        self._shapes = {}                  # ticket -> (eta_par, norm_r, beta, phi) of the requests that shape their guidance update
        self._next = 0

    def submit(self, prompt: str, class_guidance: float = 6, seed: int = 11, n_iter: int = 15, negative_prompt: Optional[str] = None,
               guidance_interval=None, eta: float = 0.0, guidance_rescale: float = 0.0, apg_eta: float = 1.0, apg_norm: float = 0.0,
               apg_momentum: float = 0.0) -> int:
        eta = schedule.check_eta(eta)
        row = schedule.check_guidance_shape(guidance_rescale, apg_eta, apg_norm, apg_momentum)
        if negative_prompt is not None and not self.mixed:
            raise ValueError("a negative prompt needs RequestBatcher(mixed=True)")
        if guidance_interval is not None and not self.mixed:
            raise ValueError("a guidance interval needs RequestBatcher(mixed=True)")
        interval = per_request_intervals(guidance_interval, 1)[0] if guidance_interval is not None else None
        ticket = self._next
        self._next += 1
        if interval is not None:
            self._intervals[ticket] = interval
        if eta > 0.0:
            self._etas[ticket] = eta
        if not schedule.guidance_shape_neutral(row):
            self._shapes[ticket] = row
        self._queue.append(_Request(ticket, str(prompt), float(class_guidance), int(seed), int(n_iter),
                                    None if negative_prompt is None else str(negative_prompt)))
        return ticket

    def pending(self) -> int:
        return len(self._queue)

    @staticmethod
    def _shape_kwargs(rows):
        """Rows ``(eta_par, norm_r, beta, phi)``, one per request of a call, as ``generate_images_from_texts``' per-prompt keyword lists."""
        return dict(apg_eta=[r[0] for r in rows], apg_norm=[r[1] for r in rows], apg_momentum=[r[2] for r in rows],
                    guidance_rescale=[r[3] for r in rows])

    @staticmethod
    def call_rows(requests) -> int:
        """Conditioning rows one mixed call of ``requests`` (``(n_iter, has_negative)`` pairs) needs: the distinct float32 noise levels of
        their schedules, one label row each, the zero row and one row per negative prompt (``tld_sample_requests``)."""
        requests = list(requests)
        sigmas = set()
        for n, _ in requests:
            sigmas.update(np.asarray(schedule.noise_schedule(int(n), 1), dtype=np.float32).tolist())
        return len(sigmas) + len(requests) + 1 + sum(1 for _, neg in requests if neg)

    def plan(self):
        """[(class_guidance, n_iter, [(ticket, prompt, seed), ...]), ...] -- the sampler calls ``flush`` will make.
        ``mixed=True``: [[(ticket, prompt, class_guidance, seed, n_iter, negative_prompt), ...], ...], in submission order."""
        if self.mixed:
            calls, cur = [], []
            for q in self._queue:
                if cur and (len(cur) == self.max_batch or
                            self.call_rows([(r.n_iter, r.negative_prompt is not None) for r in cur + [q]]) > schedule.REQUEST_ROW_CAP):
                    calls.append(cur)
                    cur = []
                cur.append(q)
            if cur:
                calls.append(cur)
            return calls
        groups = {}
        for q in self._queue:
            key = (q.class_guidance, q.n_iter, self._etas.get(q.ticket, 0.0), self._shapes.get(q.ticket, schedule.GUIDANCE_SHAPE_NEUTRAL))
            groups.setdefault(key, []).append((q.ticket, q.prompt, q.seed))
        calls = []
        for (g, n, _, _), reqs in sorted(groups.items(), key=lambda kv: -len(kv[1])):   # (a group's eta and shape are those of any of its tickets)
            for i in range(0, len(reqs), self.max_batch):
                calls.append((g, n, reqs[i:i + self.max_batch]))
        return calls

    def flush(self):
        """Run every queued request; returns {ticket: image}.  Requests leave the queue as their group completes, so a failing group
        (bad prompt, out of memory) loses nothing that was already computed: the exception carries ``partial`` = the finished images,
        and a retry only repeats the groups that did not run."""
        out = {}
        for call in self.plan():
            if self.mixed:                    # a list of the queue's records
                reqs = call
                kw = dict(class_guidance=[r.class_guidance for r in reqs], seeds=[r.seed for r in reqs], n_iter=[r.n_iter for r in reqs])
                if any(r.negative_prompt is not None for r in reqs):
                    kw["negative_prompts"] = [r.negative_prompt for r in reqs]
                if any(r.ticket in self._intervals for r in reqs):
                    kw["guidance_interval"] = [self._intervals.get(r.ticket) for r in reqs]
                if any(r.ticket in self._etas for r in reqs):
                    kw["eta"] = [self._etas.get(r.ticket, 0.0) for r in reqs]
                if any(r.ticket in self._shapes for r in reqs):
                    kw.update(self._shape_kwargs([self._shapes.get(r.ticket, schedule.GUIDANCE_SHAPE_NEUTRAL) for r in reqs]))
            else:                             # (class_guidance, n_iter, [(ticket, prompt, seed), ...])
                g, n, reqs = call
                kw = dict(class_guidance=g, seeds=[s for _, _, s in reqs], n_iter=n)
                if reqs[0][0] in self._etas:
                    kw["eta"] = self._etas[reqs[0][0]]
                if reqs[0][0] in self._shapes:
                    kw.update(self._shape_kwargs([self._shapes[reqs[0][0]]] * len(reqs)))
            try:
                imgs = self.pipeline.generate_images_from_texts([r[1] for r in reqs], **kw)
            except Exception as exc:
                exc.partial = out
                raise
            out.update({r[0]: im for r, im in zip(reqs, imgs)})
            done = {r[0] for r in reqs}
            for t in done:
                self._intervals.pop(t, None)
                self._etas.pop(t, None)
                self._shapes.pop(t, None)
            self._queue = [q for q in self._queue if q.ticket not in done]
        return out

"""Sample-sharded sampling across the GPUs of one node.

Every image's reverse-diffusion trajectory is independent (no batch statistics anywhere; CFG couples
only a sample's own cond/uncond pair, tld/diffusion.py:122-125).  Rank r of R therefore takes the
contiguous slice [r*B/R, (r+1)*B/R) of (x_T, labels), builds its CFG-doubled batch locally, runs all
steps with ZERO communication on a full weight replica, and a single all-gather (RCCL over xGMI when
the backend is "nccl") returns the final latents to every rank in the original order.  The initial
noise is drawn for the WHOLE batch with the same seed on every rank and then sliced, so results do
not depend on R.

The reference has no inference-side distribution (diffusion.py:18 single device); this is new
capability behind the unchanged ``DiffusionGenerator`` contract.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from .diffusion import per_request_intervals, stack_optional


def shard_bounds(total: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous, balanced split: the first ``total % world`` ranks get one extra item."""
    base, rem = divmod(total, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def sharded_sample(sample_fn: Callable[..., torch.Tensor], x_T: torch.Tensor,
                   labels: torch.Tensor, group: Optional[dist.ProcessGroup] = None, extras: Sequence[Optional[torch.Tensor]] = ()) -> torch.Tensor:
    """Run ``sample_fn(x_T_shard, labels_shard, *extras_shards) -> latents_shard`` on this rank's slice and all-gather.

    ``x_T`` [B,C,S,S] and ``labels`` [B,text] are the FULL batch, identical on every rank; ``extras`` are further per-sample tensors
    (leading dimension B: initial latents, masks) sliced with the same bounds -- a ``None`` entry is passed through as ``None``.
    Returns the full [B,C,S,S] latents on every rank.
    """
    extras = tuple(extras)
    for t in extras:
        if t is not None and t.shape[0] != x_T.shape[0]:
            raise ValueError(f"extras: a tensor of {t.shape[0]} samples beside x_T of {x_T.shape[0]}")
    if not (dist.is_available() and dist.is_initialized()):
        return sample_fn(x_T, labels, *extras)
    world, rank = dist.get_world_size(group), dist.get_rank(group)
    B = x_T.shape[0]
    lo, hi = shard_bounds(B, world, rank)
    mine = sample_fn(x_T[lo:hi], labels[lo:hi], *(None if t is None else t[lo:hi] for t in extras)) if hi > lo else x_T.new_zeros((0,) + tuple(x_T.shape[1:]))
    mine = mine.contiguous()
    home = mine.device
    if dist.get_backend(group) == "gloo" and mine.is_cuda:
        mine = mine.cpu()          # plumbing tests on a 1-GPU box only: gloo has no device collectives
    if B % world == 0:
        out = torch.empty((B,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
        dist.all_gather_into_tensor(out, mine, group=group)       # one collective, equal shards
        return out.to(home)
    # ragged tail: pad shards to the largest size, gather once, then trim
    per = (B + world - 1) // world
    pad = mine.new_zeros((per,) + tuple(mine.shape[1:]))
    pad[: hi - lo] = mine
    buf = torch.empty((world * per,) + tuple(mine.shape[1:]), dtype=mine.dtype, device=mine.device)
    dist.all_gather_into_tensor(buf, pad, group=group)
    parts = []
    for r in range(world):
        l2, h2 = shard_bounds(B, world, r)
        parts.append(buf[r * per: r * per + (h2 - l2)])
    return torch.cat(parts, dim=0).to(home)


def generate_latents_sharded(gen, labels: torch.Tensor, n_iter: int = 30, num_imgs: int = 16,
                             class_guidance: float = 3, seed: int = 10, img_size: int = 32, sharp_f: float = 0.1,
                             bright_f: float = 0.1, exponent: float = 1, seeds: Optional[torch.Tensor] = None,
                             noise_levels=None, use_ddpm_plus: bool = True,
                             group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """``DiffusionGenerator.generate_latents`` over all ranks of ``group`` (same arguments)."""
    x_T = gen.initialize_image(seeds, num_imgs, img_size, seed)     # full batch, same on every rank

    def one(x_shard, lab_shard):
        return gen.generate_latents(lab_shard, n_iter, x_shard.shape[0], class_guidance, seed, img_size, sharp_f, bright_f, exponent,
                                    x_shard, noise_levels, use_ddpm_plus)

    return sharded_sample(one, x_T, labels.to(x_T.device), group)


def generate_latents_from_sharded(gen, init_latents: torch.Tensor, labels: torch.Tensor, strength: float = 0.6,
                                  mask: Optional[torch.Tensor] = None, n_iter: int = 30, num_imgs: Optional[int] = None,
                                  class_guidance: float = 3, seed: int = 10, img_size: Optional[int] = None, sharp_f: float = 0.1,
                                  bright_f: float = 0.1, exponent: float = 1, seeds: Optional[torch.Tensor] = None, noise_levels=None,
                                  use_ddpm_plus: bool = True, group: Optional[dist.ProcessGroup] = None) -> torch.Tensor:
    """``DiffusionGenerator.generate_latents_from`` over all ranks of ``group`` (same arguments): every sample's noise, initial latent
    and mask travel to the rank that owns the sample."""
    num_imgs = init_latents.shape[0] if num_imgs is None else num_imgs
    img_size = init_latents.shape[-1] if img_size is None else img_size
    eps = gen.initialize_image(seeds, num_imgs, img_size, seed)     # full batch, same on every rank

    def one(eps_shard, lab_shard, z0_shard, mask_shard):
        return gen.generate_latents_from(z0_shard, lab_shard, strength, mask_shard, n_iter, eps_shard.shape[0], class_guidance, seed, img_size,
                                         sharp_f, bright_f, exponent, eps_shard, noise_levels, use_ddpm_plus)

    return sharded_sample(one, eps, labels.to(eps.device), group, extras=(init_latents, mask))


def generate_latents_requests_sharded(gen, labels: torch.Tensor, *, group: Optional[dist.ProcessGroup] = None, seed: int = 10,
                                      seeds=None, img_size: Optional[int] = None, negative_labels=None, init_latents=None, mask=None,
                                      **per_request) -> torch.Tensor:
    """``DiffusionGenerator.generate_latents_requests`` over all ranks of ``group`` (same arguments, without ``trace``).  The noise,
    labels, negative labels, initial latents and masks travel as per-sample tensors; the per-request sequences (``n_iter``,
    ``class_guidance``, ``exponent``, ``strength``, ``use_ddpm_plus``, ``eta``, ``noise_seeds``, ``guidance_rescale``, ``apg_eta``, ``apg_norm``, ``apg_momentum``) ride as the requests' indices, one more ``extras`` tensor sliced
    with the same bounds, and every rank picks its own entries.  The noise is drawn and the optional operands are stacked by the helpers
    ``generate_latents_requests`` itself uses; a whole tensor travels as it is (``sharded_sample`` checks its batch)."""
    B = labels.shape[0]
    size = gen.model.image_size if img_size is None else img_size
    eps = gen._noise(seeds, B, size, seed)                           # full batch, same on every rank
    # per-step guidance: one interval / one table per request, picked by index like the other per-request sequences (a single (lo, hi) is for all)
    if per_request.get("guidance_interval") is not None:
        per_request["guidance_interval"] = per_request_intervals(per_request["guidance_interval"], B)
    if per_request.get("guidance_schedule") is not None:
        per_request["guidance_schedule"] = list(per_request["guidance_schedule"])
    # the stochastic sampler: a request's noise key belongs to the request, so the default keys are made here, from the whole batch's seeds, and sliced
    eta = per_request.get("eta", 0.0)
    if any(float(v) > 0.0 for v in ([eta] if not isinstance(eta, (list, tuple)) else eta)):
        per_request["noise_seeds"] = gen._noise_keys(seeds, per_request.get("noise_seeds"), B, seed)

    def tensor_of(v, what, shape, fill):
        return v if isinstance(v, torch.Tensor) else stack_optional(v, what, B, shape, fill)

    has_neg = None
    if negative_labels is not None and not isinstance(negative_labels, torch.Tensor):
        has_neg = [t is not None for t in negative_labels]
    neg = tensor_of(negative_labels, "neg_labels", (labels.shape[1],), 0.0)
    z0 = tensor_of(init_latents, "init_latents", tuple(eps.shape[1:]), 0.0)
    m = tensor_of(mask, "mask", (1, size, size), 1.0)

    def one(eps_shard, lab_shard, which, neg_shard, z0_shard, mask_shard):
        w = [int(i) for i in which]
        kw = {k: (v if not isinstance(v, (list, tuple)) else [v[i] for i in w]) for k, v in per_request.items()}
        if neg_shard is not None and has_neg is not None:
            neg_shard = [neg_shard[j] if has_neg[i] else None for j, i in enumerate(w)]
        return gen.generate_latents_requests(lab_shard, negative_labels=neg_shard, seeds=eps_shard, img_size=size, init_latents=z0_shard,
                                             mask=mask_shard, **kw)

    return sharded_sample(one, eps, labels.to(eps.device), group, extras=(torch.arange(B), neg, z0, m))

"""Parameter groups of the fused optimizer step (``tld_opt_plan_*`` / ``tld_train_*_grouped``, include/tld_hip.h): the
host side.  Pure functions -- nothing here touches the device -- that turn ``torch.optim.AdamW``-style group specifications over state_dict keys
into the per-tensor tables a plan is built from, a ``LambdaLR``-style schedule into the factor table the device indexes by its own count of
APPLIED steps, and the whole back into the ``param_groups`` list of an equivalent ``torch.optim.AdamW`` for checkpoints."""
from __future__ import annotations

import math
from fnmatch import fnmatchcase
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

Group = Tuple[float, float, bool]                     # (lr_scale, weight_decay, frozen)
POS_EMBED = "denoiser_trans_block.pos_embed.weight"


def _patterns(spec: Mapping[str, object]) -> List[str]:
    m = spec.get("match")
    if isinstance(m, str):
        return [m]
    if not m or not all(isinstance(p, str) for p in m):
        raise ValueError(f"param group {dict(spec)!r}: 'match' must be a glob or a non-empty list of globs")
    return list(m)


def resolve(layout: Mapping[str, Tuple[int, Tuple[int, ...]]], param_groups: Optional[Sequence[Mapping[str, object]]],
            weight_decay: float = 0.0) -> Tuple[List[int], List[int], List[Group]]:
    """``(seg_numel, seg_group, groups)`` in ``param_layout`` order.  ``param_groups``: a list of ``dict(match=<glob or list of globs over the
    state_dict keys, fnmatch>, lr_scale=1.0, weight_decay=None, frozen=False)``; ``weight_decay=None`` inherits the default.  The FIRST spec that
    matches a tensor takes it; tensors no spec matches form the default group ``(1.0, weight_decay, False)``, which is always group 0 (spec i is
    group i + 1).  A spec whose patterns match no tensor at all raises ``ValueError`` naming it."""
    wd0 = float(weight_decay)
    if not (math.isfinite(wd0) and wd0 >= 0.0):
        raise ValueError(f"weight_decay = {weight_decay}: finite and >= 0")
    specs = list(param_groups or [])
    if len(specs) > 255:
        raise ValueError(f"{len(specs)} param groups: at most 255 beside the default one")
    groups: List[Group] = [(1.0, wd0, False)]
    pats = []
    for spec in specs:
        unknown = set(spec) - {"match", "lr_scale", "weight_decay", "frozen"}
        if unknown:
            raise ValueError(f"param group {dict(spec)!r}: unknown keys {sorted(unknown)}")
        ps = _patterns(spec)
        if not any(fnmatchcase(k, p) for k in layout for p in ps):
            raise ValueError(f"param group with match={spec.get('match')!r} matches no tensor")
        scale = float(spec.get("lr_scale", 1.0))
        wd = wd0 if spec.get("weight_decay") is None else float(spec["weight_decay"])
        if not (math.isfinite(scale) and scale >= 0.0 and math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"param group with match={spec.get('match')!r}: lr_scale and weight_decay must be finite and >= 0")
        groups.append((scale, wd, bool(spec.get("frozen", False))))
        pats.append(ps)
    seg_numel, seg_group = [], []
    for k, (_, shape) in layout.items():
        seg_numel.append(int(np.prod(shape)))
        seg_group.append(next((i + 1 for i, ps in enumerate(pats) if any(fnmatchcase(k, p) for p in ps)), 0))
    return seg_numel, seg_group, groups


def no_decay(layout: Mapping[str, Tuple[int, Tuple[int, ...]]]) -> List[Dict[str, object]]:
    """The usual exemptions as a one-spec list (so that it concatenates with further specs): every tensor of one dimension (LayerNorm affines,
    biases) and the position table keep ``weight_decay = 0``."""
    keys = [k for k, (_, shape) in layout.items() if len(shape) == 1 or k.endswith("pos_embed.weight")]
    return [dict(match=keys, weight_decay=0.0)]


def lr_table(fn_or_sequence: Union[Callable[[int], float], Sequence[float]], steps: Optional[int] = None) -> np.ndarray:
    """float32 ``table[j] = fn(j)`` for ``j < steps`` -- ``LambdaLR``'s convention: the applied step ``t = 1, 2, ...`` runs at ``fn(t - 1)``; past
    the table the last entry holds.  A sequence is taken as the table itself (``steps`` may cut it)."""
    if callable(fn_or_sequence):
        if steps is None or int(steps) < 1:
            raise ValueError("lr_table of a function needs steps >= 1")
        t = np.array([float(fn_or_sequence(j)) for j in range(int(steps))], dtype=np.float64)
    else:
        t = np.asarray(list(fn_or_sequence), dtype=np.float64).reshape(-1)
        if steps is not None:
            t = t[:int(steps)]
        if t.size == 0:
            raise ValueError("an empty lr table")
    if not bool(np.all(np.isfinite(t) & (t >= 0.0))):
        raise ValueError("lr factors must be finite and >= 0")
    return t.astype(np.float32)


def warmup_constant(warmup: int) -> Callable[[int], float]:
    """``fn(j) = min(1, (j + 1) / warmup)``: the applied step t runs at t / warmup until it reaches 1 at t = warmup."""
    w = int(warmup)
    return lambda j: 1.0 if w <= 0 else min(1.0, (int(j) + 1) / float(w))


def warmup_cosine(warmup: int, total: int, min_ratio: float = 0.0) -> Callable[[int], float]:
    """``warmup_constant(warmup)`` for ``j < warmup``, then half a cosine from 1 down to ``min_ratio`` at ``j = total - 1`` and after."""
    w, n, lo = int(warmup), int(total), float(min_ratio)

    def fn(j: int) -> float:
        j = int(j)
        if j < w:
            return (j + 1) / float(w)
        x = min(1.0, (j - w + 1) / float(max(1, n - w)))
        return lo + (1.0 - lo) * 0.5 * (1.0 + math.cos(math.pi * x))
    return fn


def torch_param_groups(seg_group: Sequence[int], groups: Sequence[Group], lr: float, betas=(0.9, 0.999), eps: float = 1e-8,
                       lr_factor: float = 1.0, scheduled: bool = False) -> List[Dict[str, object]]:
    """The ``param_groups`` list of the equivalent ``torch.optim.AdamW``: one torch group per group of ours, ``params`` by index in
    ``named_parameters()`` (= ``param_layout``) order, ``lr`` the CURRENT value ``lr * lr_scale * lr_factor`` and, with a schedule, ``initial_lr``
    as ``LambdaLR`` keeps it.  A frozen group is marked ``frozen`` (torch's counterpart is ``requires_grad = False`` on its parameters)."""
    out = []
    for q, (scale, wd, frozen) in enumerate(groups):
        g = {"lr": float(lr) * scale * float(lr_factor), "betas": tuple(betas), "eps": eps, "weight_decay": wd, "amsgrad": False, "maximize": False,
             "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": True, "lr_scale": scale,
             "frozen": bool(frozen), "params": [i for i, sq in enumerate(seg_group) if sq == q]}
        if scheduled:
            g["initial_lr"] = float(lr) * scale
        out.append(g)
    return out

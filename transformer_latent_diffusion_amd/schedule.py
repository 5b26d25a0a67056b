"""Host-side noise schedule and multistep coefficients of the sampler (float64, no device work).

Restates tld/diffusion.py:50-57 and the per-step scalar algebra of :66-83 as a table of float32
coefficients that the on-device update kernel consumes:

    x0_cfg = g * x0[:B] + (1 - g) * x0[B:]                                  (:124-125)
    D      = c1 * x0_cfg - c2 * x0_prev          (c1 = 1, c2 = 0 on the first step or DDIM; :71-79)
    x_t    = (a * D + b * x_t) / c               (a = s_i - s_{i+1}, b = s_{i+1}, c = s_i; :72,:81)

The reference evaluates those scalars as Python floats (float64) and lets torch round each one to
the tensor dtype when it meets the tensor; ``step_coefficients`` performs exactly that rounding.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import numpy as np


def _torch_arange_f32(size: int, step: float, vec: int = 8) -> np.ndarray:
    """float32 ``torch.arange(0, 1, step)`` as torch's x86 CPU kernel evaluates it.

    ATen fills the range in pairs of 8-lane vectors: each vector's base is ``float32(step * idx)``
    and lane j holds ``float32(float64(base) + j * step)``; the tail shorter than two vectors is
    ``float32(step * idx)`` per element.  The two forms differ by one float32 ulp at a few indices
    (first at n_iter=40, index 31); reproducing the 8-lane vector form keeps the schedule bit-identical
    to what the reference computed on the AVX2 ATen build the fixtures were captured with
    (tests/golden/g6_schedule.npz).  ``vec`` is the lane count of ``Vectorized<float>``: an AVX-512 ATen
    build uses 16, where the reference's own schedule differs from the fixture by at most 1 float32 ulp at
    a few indices -- harmless (sigma only feeds fp32 scalars), but the bit-exact claim is per ISA.
    """
    out = np.empty(size, dtype=np.float32)
    i = 0
    lanes = np.arange(vec, dtype=np.float64)
    while i <= size - 2 * vec:
        for h in (0, 1):
            base = np.float32(step * (i + h * vec))
            out[i + h * vec: i + (h + 1) * vec] = (np.float64(base) + lanes * step).astype(np.float32)
        i += 2 * vec
    if i < size:
        out[i:] = (np.arange(i, size, dtype=np.float64) * step).astype(np.float32)
    return out


def _torch_pow_f32(t: np.ndarray, exponent: float) -> np.ndarray:
    """float32 ``torch.pow(tensor, python_scalar)``: ATen's CPU kernel special-cases the exponents
    0.5 (sqrt), 2, 3, -0.5, -1, -2 and calls powf otherwise (ulp-level agreement of the general
    branch with a given torch build's vectorised powf is not pinned)."""
    t = t.astype(np.float32)
    if exponent == 1:
        return t
    if exponent == 0.5:
        return np.sqrt(t, dtype=np.float32)
    if exponent == 2:
        return (t * t).astype(np.float32)
    if exponent == 3:
        return (t * t * t).astype(np.float32)
    with np.errstate(divide="ignore"):
        if exponent == -0.5:
            return (np.float32(1) / np.sqrt(t, dtype=np.float32)).astype(np.float32)
        if exponent == -1:
            return (np.float32(1) / t).astype(np.float32)
        if exponent == -2:
            return (np.float32(1) / (t * t)).astype(np.float32)
        return np.power(t, np.float32(exponent), dtype=np.float32)


def noise_schedule(n_iter: int, exponent: float = 1.0,
                   noise_levels: Optional[Sequence[float]] = None) -> List[float]:
    """``(1 - arange(0, 1, 1/n_iter) ** exponent).tolist()`` with ``[0] = 0.99`` (diffusion.py:50-52).

    torch.arange(0, 1, step) with python-float arguments yields a float32 tensor of
    ``ceil((1 - 0) / step)`` entries (size computed in float64 -- hence 50 entries for n_iter=49),
    each ``float32(i * step)``; pow and the subtraction run in float32; ``.tolist()`` widens the
    float32 values to Python floats.
    """
    if noise_levels is None:
        step = 1.0 / n_iter
        size = int(math.ceil((1.0 - 0.0) / step))
        t = _torch_arange_f32(size, step)
        t = _torch_pow_f32(t, exponent)
        levels = [float(v) for v in (np.float32(1.0) - t).astype(np.float32)]
    else:
        levels = [float(v) for v in noise_levels]
    levels[0] = 0.99
    return levels


def truncate_levels(levels: Sequence[float], strength: float) -> Tuple[int, List[float]]:
    """Where an image-to-image trajectory enters the schedule: ``(k, levels[k:])`` with ``k`` the smallest index whose level is
    ``<= strength``.  ``strength`` in (0, 1]: 1.0 keeps the whole schedule (``k = 0``, the text-to-image trajectory), a small value
    keeps only its low-noise tail.  The initial latent is noised to ``levels[k]`` with the training loop's forward process
    (tld/train.py:130) and the remaining steps run unchanged, the first of them first-order (``step_coefficients`` of the tail).

    Raises ValueError for a strength outside (0, 1], below every level, or leaving fewer than the two levels a trajectory needs."""
    s = float(strength)
    if not (0.0 < s <= 1.0):
        raise ValueError(f"strength {strength!r} outside (0, 1]")
    lv = [float(v) for v in levels]
    k = next((i for i, v in enumerate(lv) if v <= s), None)
    if k is None or len(lv) - k < 2:
        raise ValueError(f"strength {s} leaves {0 if k is None else len(lv) - k} of {len(lv)} noise levels; a trajectory needs two "
                         f"(lowest levels: {lv[-2:]})")
    return k, lv[k:]


def multistep_ratios(noise_levels: Sequence[float]) -> List[float]:
    """``rs`` of diffusion.py:54-57: log-SNR lambdas, their increments hs, and hs[i-1]/hs[i].

    Raises ZeroDivisionError when a level is exactly 0.0, as the reference's Python-float division
    does (n_iter=49 hits this through the arange size quirk).
    """
    lambdas = [float(np.log((1 - float(s)) / float(s))) for s in noise_levels]
    hs = [lambdas[i] - lambdas[i - 1] for i in range(1, len(lambdas))]
    return [hs[i - 1] / hs[i] for i in range(1, len(hs))]


def check_eta(eta) -> float:
    """``eta`` of the stochastic sampler as a float: finite and >= 0, else ValueError."""
    try:
        v = float(eta)
    except (TypeError, ValueError):
        raise ValueError(f"eta = {eta!r}: expected a number")
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"eta = {eta!r}: expected a finite value >= 0")
    return v


def stochastic_step_coefficients_f64(noise_levels: Sequence[float], use_ddpm_plus: bool, eta: float) -> Tuple[np.ndarray, np.ndarray]:
    """The float64 table and noise coefficients ``step_coefficients(..., eta > 0)`` rounds to float32.

    With alpha = 1 - sigma, lambda = log(alpha / sigma), a step from level s to t, h = lambda_t - lambda_s > 0 and D = c1 x0 - c2 x0_prev:

        x_t = (sigma_t / sigma_s) e^{-eta h} x_s + alpha_t (1 - e^{-(1 + eta) h}) D + sigma_t sqrt(1 - e^{-2 eta h}) z,   z ~ N(0, I)

    the eta form of k-diffusion's ``sample_dpmpp_2m_sde`` ("midpoint") written for a general alpha; c1 = c2 + 1 = 1 + 1 / (2 r) are the
    deterministic solver's (first order on the first step, and throughout with ``use_ddpm_plus=False``: DDIM with that eta).  In the kernel's
    spelling ``x_t = (a D + b x_s) / c``: c = sigma_s, b = sigma_t e^{-eta h}, a = sigma_s alpha_t (1 - e^{-(1 + eta) h}), and the new
    e = sigma_t sqrt(1 - e^{-2 eta h}).  Both 1 - e^{-x} are evaluated as -expm1(-x).  Returns ``(table [n, 6], e [n])``; the last row is the
    final prediction's (e = 0).  Raises ValueError unless eta is finite and > 0 and the levels lie in (0, 1) and strictly decrease."""
    eta = check_eta(eta)
    nl = [float(v) for v in noise_levels]
    n = len(nl)
    if not eta > 0.0:
        raise ValueError("eta = 0 is the deterministic table: step_coefficients(levels, use_ddpm_plus)")
    if n < 2:
        raise ValueError("a trajectory needs at least two noise levels")
    if not all(math.isfinite(v) and 0.0 < v < 1.0 for v in nl):
        raise ValueError(f"eta > 0 needs every noise level inside (0, 1) (lambda = log((1 - sigma) / sigma)); have {nl}")
    if any(nl[i + 1] >= nl[i] for i in range(n - 1)):
        raise ValueError(f"eta > 0 needs strictly decreasing noise levels (h = lambda_t - lambda_s > 0); have {nl}")
    lam = [math.log((1.0 - s) / s) for s in nl]
    rs = multistep_ratios(nl) if use_ddpm_plus else None
    tab = np.zeros((n, 6), dtype=np.float64)
    e = np.zeros(n, dtype=np.float64)
    for i in range(n - 1):
        s, t = nl[i], nl[i + 1]
        h = lam[i + 1] - lam[i]
        c1, c2 = 1.0, 0.0
        if i > 0 and use_ddpm_plus:
            c1 = 1 + 1 / (2 * rs[i - 1])
            c2 = 1 / (2 * rs[i - 1])
        tab[i] = (s, s * (1.0 - t) * -math.expm1(-(1.0 + eta) * h), t * math.exp(-eta * h), s, c1, c2)
        e[i] = t * math.sqrt(-math.expm1(-2.0 * eta * h))
    tab[n - 1] = (nl[n - 1], 0.0, 0.0, 1.0, 1.0, 0.0)
    return tab, e


def step_coefficients(noise_levels: Sequence[float], use_ddpm_plus: bool = True, eta: float = 0.0):
    """float32 table [n_levels, 6] = (sigma, a, b, c, c1, c2) per forward.

    Row i < n_levels-1 drives loop iteration i (diffusion.py:66-83); the last row is the final
    prediction at ``next_noise`` of the last iteration (:85), for which only sigma is meaningful.

    ``eta`` (not in the reference): 0 returns this table, from this code.  ``eta > 0`` returns ``(table, e)``: the
    table of the SDE solver (``stochastic_step_coefficients_f64``) and the float32 vector ``e`` [n_levels] of the noise added after each
    step's update, 0 for the final prediction.  A negative or non-finite eta, or with eta > 0 levels that do not strictly decrease inside
    (0, 1), raise ValueError before anything else.
    """
    eta = check_eta(eta)
    if eta > 0.0:
        tab64, e64 = stochastic_step_coefficients_f64(noise_levels, use_ddpm_plus, eta)
        return tab64.astype(np.float32), e64.astype(np.float32)
    nl = [float(v) for v in noise_levels]
    n = len(nl)
    if n < 2:
        # the reference would hit an unbound ``next_noise`` at diffusion.py:85
        raise UnboundLocalError("generate() needs at least two noise levels")
    rs = multistep_ratios(nl) if use_ddpm_plus else None
    tab = np.zeros((n, 6), dtype=np.float64)
    for i in range(n - 1):
        curr, nxt = nl[i], nl[i + 1]
        c1, c2 = 1.0, 0.0
        if i > 0 and use_ddpm_plus:
            c1 = 1 + 1 / (2 * rs[i - 1])
            c2 = 1 / (2 * rs[i - 1])
        tab[i] = (curr, curr - nxt, nxt, curr, c1, c2)
    tab[n - 1] = (nl[n - 1], 0.0, 0.0, 1.0, 1.0, 0.0)
    return tab.astype(np.float32)


# ---- B requests in one sampler call (tld_sample_requests): the host planning, held against the engine's (csrc/tld_sample_plan.h) by tests/test_sample_plan_host.py ----
REQUEST_ROW_CAP = 1024      # most conditioning rows one call may need: kMaxRequestCondRows in csrc/tld_sample_plan.h


def request_order(level_counts: Sequence[int]) -> List[int]:
    """Order in which the engine takes the requests: by descending level count, stable (equal counts keep the caller's order), so that the
    requests still running at step i are a prefix.  ``order[k]`` is the caller's index of the k-th record."""
    return sorted(range(len(level_counts)), key=lambda b: -int(level_counts[b]))


def active_prefix(sorted_counts: Sequence[int]) -> List[int]:
    """``B_i = #{b : n_levels[b] > i}`` for i = 0 .. n_max - 1 of counts in non-increasing order: the model runs ``2 B_i`` samples at step i."""
    counts = [int(c) for c in sorted_counts]
    if any(counts[k] < counts[k + 1] for k in range(len(counts) - 1)):
        raise ValueError(f"level counts {counts} are not in non-increasing order")
    return [sum(1 for c in counts if c > i) for i in range(counts[0] if counts else 0)]


def distinct_sigma_rows(coeff_list: Sequence[np.ndarray]) -> Tuple[np.ndarray, List[List[int]]]:
    """Noise rows of a call: the float32 sigmas of every (request, step) deduplicated BY VALUE (bit pattern), in order of first use walking
    step by step over the requests as given -- the engine's order when they are sorted (``request_order``).  Returns ``(sigmas, rows)`` with
    ``rows[b][i]`` the row of request b at step i; requests that share a schedule share rows."""
    tabs = [np.ascontiguousarray(c, dtype=np.float32) for c in coeff_list]
    seen, sigmas = {}, []
    rows = [[0] * t.shape[0] for t in tabs]
    for i in range(max((t.shape[0] for t in tabs), default=0)):
        for b, t in enumerate(tabs):
            if i < t.shape[0]:
                key = t[i, 0].tobytes()
                if key not in seen:
                    seen[key] = len(sigmas)
                    sigmas.append(t[i, 0])
                rows[b][i] = seen[key]
    return np.array(sigmas, dtype=np.float32), rows


def request_cond_rows(coeff_list: Sequence[np.ndarray], n_negative: int = 0) -> int:
    """Conditioning rows a call of these requests needs: distinct sigmas + one label row each + the zero row + one per negative label."""
    return len(distinct_sigma_rows(coeff_list)[0]) + len(coeff_list) + 1 + int(n_negative)


# ---- one guidance value per forward (tld_sample_requests_guided) ---------------------------------------------------------
def guidance_table(coeffs: np.ndarray, class_guidance: float, interval: Optional[Tuple[float, float]] = None) -> np.ndarray:
    """float32 [n_levels]: a request's guidance per forward under limited-interval guidance -- ``class_guidance`` where the forward's noise
    level lies inside ``interval = (lo, hi)`` (both edges inclusive), else exactly 1.0, the value at which the engine runs no unconditional
    sample.  The level of forward i is column 0 of ``step_coefficients``, the float32 sigma the model is conditioned on, and the comparison
    is made in float32; the last entry belongs to the final prediction.  ``interval`` None: guided throughout."""
    sig = np.ascontiguousarray(coeffs, dtype=np.float32)
    if sig.ndim != 2 or sig.shape[1] != 6:
        raise ValueError(f"coeffs {sig.shape}: expected [n_levels, 6]")
    g = np.float32(class_guidance)
    if not np.isfinite(g):
        raise ValueError(f"class_guidance = {class_guidance} is not finite")
    if interval is None:
        return np.full(sig.shape[0], g, dtype=np.float32)
    lo, hi = (np.float32(v) for v in interval)
    if not (lo <= hi):
        raise ValueError(f"guidance interval ({interval[0]}, {interval[1]}): expected lo <= hi")
    inside = (sig[:, 0] >= lo) & (sig[:, 0] <= hi)
    return np.where(inside, g, np.float32(1.0)).astype(np.float32)


# ---- noise inside the step (tld_sample_requests_stochastic) ---------------------------------------------------------------
def noise_key(seed: int, index: int = 0) -> int:
    """A request's default 64-bit noise key: ``(seed & 0xffffffff) | (index << 32)``, ``index`` the image's place inside the ``torch.randn`` draw
    that made its start noise -- b under one batch seed, 0 where each request has its own seed.  A one-image call with seed s and the request
    "seed s" of a batched call then share the key, as they share the start noise."""
    return (int(seed) & 0xFFFFFFFF) | ((int(index) & 0xFFFFFFFF) << 32)


# ---- the shape of the guidance update (tld_sample_requests_shaped) ----------------------------------------------------------
GUIDANCE_SHAPE_NEUTRAL = (1.0, 0.0, 0.0, 0.0)       # (eta_par, norm_r, beta, phi): plain classifier-free guidance


def check_guidance_shape(guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0) -> Tuple[float, float, float, float]:
    """The four controls of the guidance update as the engine's row ``(eta_par, norm_r, beta, phi)`` of float32 values held as floats:
    ``guidance_rescale`` = phi in [0, 1] (Lin et al. 2023; 0 off), ``apg_eta`` = eta_par >= 0 (weight of the update's part parallel to the
    conditional prediction; 1 off), ``apg_norm`` = norm_r >= 0 (the update's norm is clipped to it; 0 off), ``apg_momentum`` = beta with
    |beta| < 1 (Sadat et al. 2024 use negative values; 0 off).  Anything else, a non-finite value included, raises ValueError.  The checks
    run on the float32 values, which are what the engine checks again."""
    out = []
    for name, v in (("apg_eta", apg_eta), ("apg_norm", apg_norm), ("apg_momentum", apg_momentum), ("guidance_rescale", guidance_rescale)):
        try:
            with np.errstate(over="ignore"):
                f = float(np.float32(float(v)))
        except (TypeError, ValueError, OverflowError):
            raise ValueError(f"{name} = {v!r}: expected a number")
        if not math.isfinite(f):
            raise ValueError(f"{name} = {v!r}: expected a finite value")
        out.append(f)
    eta_par, norm_r, beta, phi = out
    if eta_par < 0.0:
        raise ValueError(f"apg_eta = {apg_eta!r}: expected >= 0")
    if norm_r < 0.0:
        raise ValueError(f"apg_norm = {apg_norm!r}: expected >= 0 (0: no clipping)")
    if not abs(beta) < 1.0:
        raise ValueError(f"apg_momentum = {apg_momentum!r}: expected |beta| < 1")
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"guidance_rescale = {guidance_rescale!r}: expected inside [0, 1]")
    return eta_par, norm_r, beta, phi


def guidance_shape_neutral(row) -> bool:
    """True where the row asks for none of the four controls: the request takes plain CFG, the arithmetic of every other entry."""
    return tuple(float(v) for v in row) == GUIDANCE_SHAPE_NEUTRAL


def guidance_shape_rows(B: int, guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0):
    """Each control a scalar (for all) or a length-B sequence -> B checked rows, or None where every row is neutral (the call without ``shape``)."""
    def seq(v, name):
        if isinstance(v, (list, tuple, np.ndarray)):
            if len(v) != B:
                raise ValueError(f"{name}: {len(v)} entries for {B} requests")
            return list(v)
        return [v] * B
    cols = [seq(guidance_rescale, "guidance_rescale"), seq(apg_eta, "apg_eta"), seq(apg_norm, "apg_norm"), seq(apg_momentum, "apg_momentum")]
    rows = [check_guidance_shape(cols[0][b], cols[1][b], cols[2][b], cols[3][b]) for b in range(B)]
    return None if all(guidance_shape_neutral(r) for r in rows) else rows


def guided_rows(sorted_counts: Sequence[int], tables: Sequence[np.ndarray], skip: bool = True):
    """The model batches of a guided call, as the engine plans them: requests in the engine's order (``request_order``) with one guidance
    table each.  Returns ``(U, slots, src)`` with, per step i over the ``B_i`` requests still running (``active_prefix``): ``U[i]`` the
    number of unconditional samples, ``slots[i][b]`` the place of request b's among them (compacted in request order) or -1 where
    ``tables[b][i]`` is exactly 1.0 and it has none, and ``src[i]`` the request each of the ``B_i + U[i]`` model samples reads -- the
    identity, then the guided requests.  The call makes ``sum(counts) + sum(U)`` model-sample forwards and needs an engine of
    ``max(B_i + U[i])`` samples.  ``skip`` False (the engine under ``TLD_GUIDANCE_SKIP=0``): every request keeps its unconditional sample."""
    prefix = active_prefix(sorted_counts)
    tabs = [np.ascontiguousarray(t, dtype=np.float32) for t in tables]
    if len(tabs) != len(sorted_counts):
        raise ValueError(f"{len(tabs)} guidance tables for {len(sorted_counts)} requests")
    for b, t in enumerate(tabs):
        if t.ndim != 1 or t.shape[0] != int(sorted_counts[b]):
            raise ValueError(f"guidance table {b} {t.shape}: expected [{int(sorted_counts[b])}], one value per forward")
    U, slots, src = [], [], []
    for i, Bi in enumerate(prefix):
        guided = [b for b in range(Bi) if not skip or tabs[b][i] != np.float32(1.0)]
        place = {b: k for k, b in enumerate(guided)}
        U.append(len(guided))
        slots.append([place.get(b, -1) for b in range(Bi)])
        src.append(list(range(Bi)) + guided)
    return U, slots, src

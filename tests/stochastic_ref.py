"""CPU reference of the stochastic sampler, for tests/test_stochastic_host.py and tests/test_gpu_stochastic.py:
the numpy statement of the noise's counter layout (csrc/tld_sampler_noise.h) on tests/batch_prep_ref.py's Philox, the float64 Box-Muller of its
words, an independently written k-diffusion-form step, and tests/guided_ref.py's loop with eta and a GIVEN z."""
import math

import numpy as np
import torch

import batch_prep_ref as P
from img2img_ref import blend

NOISE_TAG = 0x534E5A31        # SAMPLER_NOISE_TAG


def noise_words(key, step, n_elems, first_quad=0):
    """Philox words of elements [4 first_quad, 4 first_quad + n_elems) of a request's image at forward ``step`` under ``key``: [ceil(n / 4), 4] uint32.
    Counter (quad, step, tag, 0), key (low word, high word)."""
    quads = np.arange(first_quad, first_quad + (n_elems + 3) // 4, dtype=np.uint64)
    assert (quads < (1 << 32)).all()
    ctr = np.empty(quads.shape + (4,), dtype=np.uint32)
    ctr[:, 0] = quads
    ctr[:, 1] = int(step) & 0xFFFFFFFF
    ctr[:, 2] = NOISE_TAG
    ctr[:, 3] = 0
    return P.philox4x32_10(ctr, np.array([int(key) & 0xFFFFFFFF, (int(key) >> 32) & 0xFFFFFFFF], dtype=np.uint32))


def noise_f64(key, step, n_elems):
    """Box-Muller in float64 on those words: elements 4 q .. 4 q + 3 from (r0, r1) and (r2, r3), u = ((r >> 8) + 0.5) 2^-24 unrounded."""
    w = noise_words(key, step, n_elems)
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    out = np.empty((w.shape[0], 4), dtype=np.float64)
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        out[:, 2 * h] = rad * np.cos(2.0 * np.pi * u[:, 2 * h + 1])
        out[:, 2 * h + 1] = rad * np.sin(2.0 * np.pi * u[:, 2 * h + 1])
    return out.reshape(-1)[:n_elems]


def kdiffusion_step(x, denoised, old_denoised, sig_s, sig_t, sig_prev, eta, z):
    """One step of k-diffusion's ``sample_dpmpp_2m_sde`` (solver_type "midpoint", s_noise 1) carried to alpha = 1 - sigma: the variance-exploding
    state is x / alpha at sigma / alpha.  float64 arrays; ``old_denoised`` / ``sig_prev`` None on the first step (or for DDIM: first order)."""
    ve = lambda s: s / (1.0 - s)
    t, t_next = -math.log(ve(sig_s)), -math.log(ve(sig_t))
    h = t_next - t
    eta_h = eta * h
    xh = x / (1.0 - sig_s)
    xh = ve(sig_t) / ve(sig_s) * math.exp(-eta_h) * xh + -math.expm1(-h - eta_h) * denoised
    if old_denoised is not None:
        r = (t - -math.log(ve(sig_prev))) / h
        xh = xh + 0.5 * -math.expm1(-h - eta_h) * (1.0 / r) * (denoised - old_denoised)
    if eta:
        xh = xh + z * ve(sig_t) * math.sqrt(-math.expm1(-2.0 * eta_h))
    return (1.0 - sig_t) * xh


@torch.no_grad()
def sample_requests(ref, eps, z0, mask, labels, neg_labels, levels_list, start_mix, g, use_ddpm_plus, eta, z, sharp_f=0.0, bright_f=0.0, trace=False):
    """``guided_ref.sample_requests`` with ``eta``: B values, and ``z``: ``z[b][i]`` the [C,S,S] normals request b adds after the update of its
    forward i (read where ``eta[b] > 0`` only).  A request with eta 0 runs guided_ref's arithmetic, operation for operation."""
    B = eps.shape[0]
    nls = [[float(v) for v in lv] for lv in levels_list]
    n_max = max(len(nl) for nl in nls)
    neg = torch.stack([torch.zeros_like(labels[b]) if neg_labels is None or neg_labels[b] is None else neg_labels[b] for b in range(B)])
    lams = [[math.log((1 - s) / s) for s in nl] for nl in nls]
    rs = []
    for b, nl in enumerate(nls):
        if use_ddpm_plus[b]:
            hs = [lams[b][i] - lams[b][i - 1] for i in range(1, len(nl))]
            rs.append([hs[i - 1] / hs[i] for i in range(1, len(hs))])
        else:
            rs.append(None)
    x_t = [eps[b].clone() if start_mix[b] == 1.0 else start_mix[b] * eps[b] + (1 - start_mix[b]) * z0[b] for b in range(B)]
    x0_prev = [None] * B
    out = torch.zeros_like(eps)
    tx0 = torch.zeros((n_max - 1,) + tuple(eps.shape))
    txt = torch.zeros_like(tx0)
    for i in range(n_max):
        for b in [b for b in range(B) if len(nls[b]) > i]:
            xb = x_t[b].unsqueeze(0)
            x0_2 = ref.forward(torch.cat([xb, xb]), torch.full((2, 1), nls[b][i]), torch.stack([labels[b], neg[b]]))
            gi = float(g[b][i])
            x0 = x0_2[0].clone() if gi == 1.0 else gi * x0_2[0] + (1 - gi) * x0_2[1]
            nl = nls[b]
            if i == len(nl) - 1:
                if mask is not None:
                    x0 = blend(mask[b], x0, z0[b])
                x0[3] += sharp_f
                x0[0] += bright_f
                out[b] = x0
                continue
            cur, nxt = nl[i], nl[i + 1]
            if i == 0 or not use_ddpm_plus[b]:
                D = x0
            else:
                D = (1 + 1 / (2 * rs[b][i - 1])) * x0 - (1 / (2 * rs[b][i - 1])) * x0_prev[b]
            et = float(eta[b])
            if et == 0.0:
                xt = ((cur - nxt) * D + nxt * x_t[b]) / cur
            else:
                h = lams[b][i + 1] - lams[b][i]
                xt = (nxt / cur) * math.exp(-et * h) * x_t[b] + (1 - nxt) * -math.expm1(-(1 + et) * h) * D
                xt = xt + nxt * math.sqrt(-math.expm1(-2 * et * h)) * z[b][i]
            if mask is not None:
                xt = blend(mask[b], xt, nxt * eps[b] + (1 - nxt) * z0[b])
            x_t[b], x0_prev[b] = xt, x0
            tx0[i, b], txt[i, b] = x0, xt
    return (out, tx0, txt) if trace else out

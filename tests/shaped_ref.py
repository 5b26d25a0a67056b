"""CPU reference of the shaped guidance update, for tests/test_guidance_shape_host.py and tests/test_gpu_guidance_shape.py:
the numpy statement of csrc/tld_guidance_shape.h (five sums -> two fp32 weights -> one fma), the DIRECT float64 statement it stands for (project,
clip, rescale by the standard deviations: no sums of products, no algebra), and tests/stochastic_ref.py's loop with a shape row per request."""
import math

import numpy as np
import torch

from img2img_ref import blend

NEUTRAL = (1.0, 0.0, 0.0, 0.0)        # (eta_par, norm_r, beta, phi)


def is_neutral(row):
    return tuple(float(np.float32(v)) for v in row) == NEUTRAL


def dbar_f32(c, u, m, beta):
    """fl32(c - u), then with beta != 0 fl32(d + fl32(beta m)): float32 arrays, every operation rounded."""
    c, u = np.asarray(c, np.float32), np.asarray(u, np.float32)
    d = c - u
    beta = np.float32(beta)
    if beta != 0:
        d = d + beta * np.asarray(m, np.float32)
    assert d.dtype == np.float32
    return d


def sums_f64(c, dbar):
    """(Sc, Sd, Scc, Sdc, Sdd) by math.fsum over the float32 operands: the exactly rounded sums."""
    c, d = np.asarray(c, np.float64).ravel(), np.asarray(dbar, np.float64).ravel()
    return [math.fsum(c), math.fsum(d), math.fsum(c * c), math.fsum(d * c), math.fsum(d * d)]


def abs_sums_f64(c, dbar):
    """sum |term| of the same five sums: the scale of their error bound."""
    c, d = np.abs(np.asarray(c, np.float64).ravel()), np.abs(np.asarray(dbar, np.float64).ravel())
    return [math.fsum(c), math.fsum(d), math.fsum(c * c), math.fsum(d * c), math.fsum(d * d)]


def finalize(sums, n, g, row, round32=True):
    """guidance_shape_finalize of the header, operation for operation in float64 -> (P, Q) as np.float32 (``round32`` off: the float64 products)."""
    Sc, Sd, Scc, Sdc, Sdd = (float(v) for v in sums)
    eta_par, norm_r, beta, phi = (float(np.float32(v)) for v in row)
    gm1, nn = float(np.float32(g)) - 1.0, float(n)
    s = 1.0
    if norm_r > 0.0 and Sdd > 0.0:
        q = norm_r / math.sqrt(Sdd)
        s = q if q < 1.0 else 1.0
    p = s * Sdc / Scc if Scc > 0.0 else 0.0
    A = 1.0 + gm1 * (eta_par - 1.0) * p
    B = gm1 * s
    k = 1.0
    if phi != 0.0:
        vc = Scc - Sc * Sc / nn
        mx = A * Sc + B * Sd
        vx = A * A * Scc + 2.0 * A * B * Sdc + B * B * Sdd - mx * mx / nn
        if vc > 0.0 and vx > 0.0:
            k = phi * math.sqrt(vc / vx) + (1.0 - phi)
    return (np.float32(k * A), np.float32(k * B)) if round32 else (k * A, k * B)


def weights_AB(sums, g, row):
    """(A, B) of the statement in float64 (tests pick inputs on |A|)."""
    Sc, Sd, Scc, Sdc, Sdd = (float(v) for v in sums)
    eta_par, norm_r = float(np.float32(row[0])), float(np.float32(row[1]))
    s = min(1.0, norm_r / math.sqrt(Sdd)) if norm_r > 0.0 and Sdd > 0.0 else 1.0
    p = s * Sdc / Scc if Scc > 0.0 else 0.0
    return 1.0 + (float(np.float32(g)) - 1.0) * (eta_par - 1.0) * p, (float(np.float32(g)) - 1.0) * s


def fma_f32(a, b, c):
    """fl32(a b + c) for float32 arrays, rounded once.  a b is exact in float64; the float64 sum is made round-to-odd with the error term of
    TwoSum, after which the rounding to float32 is that of the exact value (53 >= 2 * 24 + 2 bits)."""
    p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32).astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (err != 0) & even & np.isfinite(s)
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def statement(c, u, m, g, row):
    """The step's arithmetic on one request: float32 c, u (any shape), momentum m (or None: zeros) -> dict(x0, dbar, sums, P, Q).  The sums are the
    exactly rounded ones (math.fsum), standing for the kernel's double accumulation."""
    c = np.asarray(c, np.float32)
    db = dbar_f32(c, u, np.zeros_like(c) if m is None else m, row[2])
    sums = sums_f64(c, db)
    P, Q = finalize(sums, c.size, g, row)
    return dict(x0=fma_f32(P, c, Q * db), dbar=db, sums=sums, P=P, Q=Q)


def direct_f64(c, dbar, g, row):
    """What the weights stand for, in float64 on the given update dbar (the roundings of d and of the momentum are part of its definition): clip
    the update's norm to norm_r, split it along the unit vector of c, weight the parallel part, add to c, then pull the standard deviation towards
    that of c by phi (torch.std).  No sums of products beyond the norms and the one dot product of a projection."""
    c = torch.as_tensor(np.asarray(c, np.float64)).reshape(-1)
    d = torch.as_tensor(np.asarray(dbar, np.float64)).reshape(-1)
    eta_par, norm_r, _, phi = (float(np.float32(v)) for v in row)
    g = float(np.float32(g))
    if norm_r > 0.0:
        nd = float(torch.linalg.vector_norm(d))
        if nd > 0.0:
            d = d * min(1.0, norm_r / nd)
    nc = float(torch.linalg.vector_norm(c))
    if nc > 0.0:
        unit = c / nc
        par = torch.dot(d, unit) * unit
    else:
        par = torch.zeros_like(d)
    orth = d - par
    x = c + (g - 1.0) * (orth + eta_par * par)
    if phi != 0.0:
        sc, sx = float(torch.std(c)), float(torch.std(x))
        if sc > 0.0 and sx > 0.0:
            x = x * (phi * (sc / sx) + (1.0 - phi))
    return x.numpy()


@torch.no_grad()
def sample_requests(ref, eps, z0, mask, labels, neg_labels, levels_list, start_mix, g, use_ddpm_plus, eta, z, shape, sharp_f=0.0, bright_f=0.0,
                    trace=False, dtype=torch.float32):
    """``stochastic_ref.sample_requests`` with ``shape``: B rows (eta_par, norm_r, beta, phi).  A request with a neutral row runs stochastic_ref's
    arithmetic, operation for operation; any other takes the direct statement above in ``dtype`` arithmetic at every forward whose guidance is not
    exactly 1.0 (those run no unconditional sample: x0 = cond, the momentum untouched).  ``dtype`` float64: the model's float32 outputs and the
    loop's state are carried in float64."""
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
    cast = lambda t: t.to(dtype)
    eps_, z0_ = cast(eps), None if z0 is None else cast(z0)
    x_t = [eps_[b].clone() if start_mix[b] == 1.0 else start_mix[b] * eps_[b] + (1 - start_mix[b]) * z0_[b] for b in range(B)]
    x0_prev = [None] * B
    mom = [torch.zeros_like(eps_[b]) for b in range(B)]
    out = torch.zeros_like(eps_)
    tx0 = torch.zeros((n_max - 1,) + tuple(eps.shape), dtype=dtype)
    txt = torch.zeros_like(tx0)
    for i in range(n_max):
        for b in [b for b in range(B) if len(nls[b]) > i]:
            xb = x_t[b].unsqueeze(0).to(torch.float32)
            x0_2 = cast(ref.forward(torch.cat([xb, xb]), torch.full((2, 1), nls[b][i]), torch.stack([labels[b], neg[b]])))
            gi = float(g[b][i])
            if gi == 1.0:
                x0 = x0_2[0].clone()
            elif is_neutral(shape[b]):
                x0 = gi * x0_2[0] + (1 - gi) * x0_2[1]
            else:
                eta_par, norm_r, beta, phi = (float(np.float32(v)) for v in shape[b])
                c, d = x0_2[0], x0_2[0] - x0_2[1]
                if beta != 0.0:
                    d = d + beta * mom[b]
                    mom[b] = d
                if norm_r > 0.0:
                    nd = float(torch.linalg.vector_norm(d.double()))
                    if nd > 0.0:
                        d = d * min(1.0, norm_r / nd)
                nc = float(torch.linalg.vector_norm(c.double()))
                unit = c / nc if nc > 0.0 else torch.zeros_like(c)
                par = (d * unit).sum() * unit
                x0 = c + (gi - 1.0) * ((d - par) + eta_par * par)
                if phi != 0.0:
                    sc, sx = float(torch.std(c)), float(torch.std(x0))
                    if sc > 0.0 and sx > 0.0:
                        x0 = x0 * (phi * (sc / sx) + (1.0 - phi))
            nl = nls[b]
            if i == len(nl) - 1:
                if mask is not None:
                    x0 = blend(cast(mask[b]), x0, z0_[b])
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
                xt = xt + nxt * math.sqrt(-math.expm1(-2 * et * h)) * cast(z[b][i])
            if mask is not None:
                xt = blend(cast(mask[b]), xt, nxt * eps_[b] + (1 - nxt) * z0_[b])
            x_t[b], x0_prev[b] = xt, x0
            tx0[i, b], txt[i, b] = x0, xt
    return (out, tx0, txt) if trace else out

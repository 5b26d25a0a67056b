"""CPU reference of the per-step-guidance sampler: tests/requests_ref.py's loop with one guidance value per
(request, forward).  A forward whose value is exactly 1.0 takes the conditional prediction itself, no arithmetic; the model still runs on the
request's (conditional, unconditional) pair there, because torch's CPU matmul moves by an ulp with the batch size (requests_ref.py).  Test
infrastructure: imported by tests/test_guidance_host.py and tests/test_gpu_guidance.py."""
import math

import torch

from img2img_ref import blend


@torch.no_grad()
def sample_requests(ref, eps, z0, mask, labels, neg_labels, levels_list, start_mix, g, use_ddpm_plus, sharp_f=0.0, bright_f=0.0, trace=False):
    """As ``requests_ref.sample_requests``, with ``g``: B sequences, ``g[b][i]`` the guidance of request b's forward i (``len(levels_list[b])``
    values, the last one the final prediction's)."""
    B = eps.shape[0]
    nls = [[float(v) for v in lv] for lv in levels_list]
    n_max = max(len(nl) for nl in nls)
    for b in range(B):
        assert len(g[b]) == len(nls[b]), f"request {b}: {len(g[b])} guidance values for {len(nls[b])} forwards"
    neg = torch.stack([torch.zeros_like(labels[b]) if neg_labels is None or neg_labels[b] is None else neg_labels[b] for b in range(B)])
    rs = []
    for b, nl in enumerate(nls):
        if use_ddpm_plus[b]:
            lam = [math.log((1 - s) / s) for s in nl]
            hs = [lam[i] - lam[i - 1] for i in range(1, len(lam))]
            rs.append([hs[i - 1] / hs[i] for i in range(1, len(hs))])
        else:
            rs.append(None)
    x_t = [eps[b].clone() if start_mix[b] == 1.0 else start_mix[b] * eps[b] + (1 - start_mix[b]) * z0[b] for b in range(B)]
    x0_prev = [None] * B
    out = torch.zeros_like(eps)
    tx0 = torch.zeros((n_max - 1,) + tuple(eps.shape))
    txt = torch.zeros_like(tx0)
    for i in range(n_max):
        act = [b for b in range(B) if len(nls[b]) > i]            # a finished request is not computed again
        for b in act:
            xb = x_t[b].unsqueeze(0)
            x0_2 = ref.forward(torch.cat([xb, xb]), torch.full((2, 1), nls[b][i]), torch.stack([labels[b], neg[b]]))
            gi = float(g[b][i])
            x0 = x0_2[0].clone() if gi == 1.0 else gi * x0_2[0] + (1 - gi) * x0_2[1]
            nl = nls[b]
            if i == len(nl) - 1:                                  # the request's final prediction
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
            xt = ((cur - nxt) * D + nxt * x_t[b]) / cur
            if mask is not None:
                xt = blend(mask[b], xt, nxt * eps[b] + (1 - nxt) * z0[b])
            x_t[b], x0_prev[b] = xt, x0
            tx0[i, b], txt[i, b] = x0, xt
    return (out, tx0, txt) if trace else out

"""CPU reference of the image-to-image / inpainting sampler: ``TorchRefDenoiser.sample``'s loop
(oracle/torch_ref.py, the restatement of tld/diffusion.py:54-92 that g2 pins to the reference) plus the three steps the feature
defines -- the noised start, the blend after every update and the blend of the final prediction.  fp32 tensors meet float64
Python scalars, as in the reference.  Test infrastructure: imported by tests/test_img2img_host.py and tests/test_gpu_img2img.py."""
import math

import torch


def blend(m, a, b):
    """m a + (1 - m) b: exact at m = 1 (a) and m = 0 (b)."""
    return m * a + (1 - m) * b


@torch.no_grad()
def sample_from(ref, eps, z0, mask, labels, levels, start_mix, g, use_ddpm_plus=True, sharp_f=0.0, bright_f=0.0, trace=False):
    """ref: TorchRefDenoiser; eps / z0 [B,C,S,S]; mask [B,1,S,S] or None; levels: the REMAINING noise levels; start_mix: s0, or 1.0
    for the pure-noise start.  Returns the end latent (with ``trace``: also the per-step unblended predictions and blended x_t)."""
    nl = [float(v) for v in levels]
    x_t = eps.clone() if start_mix == 1.0 else start_mix * eps + (1 - start_mix) * z0
    labels2 = torch.cat([labels, torch.zeros_like(labels)])
    if use_ddpm_plus:
        lam = [math.log((1 - s) / s) for s in nl]
        hs = [lam[i] - lam[i - 1] for i in range(1, len(lam))]
        rs = [hs[i - 1] / hs[i] for i in range(1, len(hs))]
    x0_prev = None
    tx0, txt = [], []

    def pred(x_in, sigma):
        b = x_in.shape[0]
        x0 = ref.forward(torch.cat([x_in, x_in]), torch.full((2 * b, 1), sigma), labels2)
        return g * x0[:b] + (1 - g) * x0[b:]

    for i in range(len(nl) - 1):
        cur, nxt = nl[i], nl[i + 1]
        x0 = pred(x_t, cur)
        if i == 0 or not use_ddpm_plus:
            D = x0
        else:
            D = (1 + 1 / (2 * rs[i - 1])) * x0 - (1 / (2 * rs[i - 1])) * x0_prev
        x_t = ((cur - nxt) * D + nxt * x_t) / cur
        if mask is not None:
            x_t = blend(mask, x_t, nxt * eps + (1 - nxt) * z0)
        x0_prev = x0
        tx0.append(x0)
        txt.append(x_t)
    x0 = pred(x_t, nl[-1])
    if mask is not None:
        x0 = blend(mask, x0, z0)
    x0[:, 3] += sharp_f
    x0[:, 0] += bright_f
    return (x0, torch.stack(tx0), torch.stack(txt)) if trace else x0

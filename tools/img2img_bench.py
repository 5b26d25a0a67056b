#!/usr/bin/env python3
"""Cost of image-to-image and inpainting beside plain text-to-image sampling at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents,
64 images, 35 noise levels, DPM-Solver++(2M), guidance 6), in one process:
    plain      DiffusionGenerator.generate_latents                             35 steps
    img2img    generate_latents_from at strength 0.6                           the levels <= 0.6 only, the step kernel without a mask
    inpaint    generate_latents_from at strength 1.0 with a half-image mask    35 steps, the step kernel with the blend
Reports the median ms per call and the `update` class time per launch (HIP events, Denoiser.get_profile); one JSON line at the end.
    python tools/img2img_bench.py [--batch 64] [--n-iter 35] [--iters 5] [--json out.json]"""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator, config_100m, schedule  # noqa: E402
from transformer_latent_diffusion_amd.weights import synth_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--n-iter", type=int, default=35)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = config_100m(32)
m = Denoiser(**asdict(cfg)).to(dev)
m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 5).items()})
gen = DiffusionGenerator(m, None, dev, torch.float32)
B, S = args.batch, 32
g = torch.Generator().manual_seed(11)
eps = torch.randn(B, 4, S, S, generator=g).to(dev)
z0 = (torch.randn(B, 4, S, S, generator=g) * 0.5).to(dev)
labels = (torch.randn(B, 768, generator=g) * 0.5).to(dev)
mask = torch.zeros(B, 1, S, S)
mask[..., : S // 2] = 1                       # regenerate the left half
mask = mask.to(dev)
kw = dict(n_iter=args.n_iter, class_guidance=6, sharp_f=0.0, bright_f=0.0, exponent=1, seeds=eps)
full = schedule.noise_schedule(args.n_iter, 1)
runs = {
    "plain": (lambda: gen.generate_latents(labels, num_imgs=B, img_size=S, **kw), len(full)),
    "img2img_0.6": (lambda: gen.generate_latents_from(z0, labels, strength=0.6, **kw), len(schedule.truncate_levels(full, 0.6)[1])),
    "inpaint_half": (lambda: gen.generate_latents_from(z0, labels, strength=1.0, mask=mask, **kw), len(full)),
}
res = {"batch": B, "n_iter": args.n_iter}
for name, (run, n_levels) in runs.items():
    run(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    m.reserve_profile("update", n_levels)
    m.set_profile(["update"]); run(); ms, n = m.get_profile("update"); m.set_profile(())
    assert n == n_levels, (name, n, n_levels)
    res[name] = {"ms_per_call": round(t * 1e3, 2), "levels": n_levels, "ms_per_step": round(t * 1e3 / n_levels, 3),
                 "update_us_per_launch": round(ms / n * 1e3, 2), "update_launches": n}
    print(f"{name:13s} {t * 1e3:8.1f} ms per call, {n_levels} levels ({t * 1e3 / n_levels:.3f} ms per step); update class {ms / n * 1e3:.1f} us per launch x {n}")
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

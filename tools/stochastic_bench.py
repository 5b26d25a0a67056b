#!/usr/bin/env python3
"""The stochastic sampler beside the deterministic call, at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents, 64 images, 35 steps, guidance 6)
in one process, at the sampler level (no text encoder, no VAE).  Three arms, the same start noise and labels:
    generate_latents   tld_sample, the yardstick
    eta0_new_entry     the same trajectory through tld_sample_requests_stochastic with all-zero noise coefficients: the slots
                       flavour of the step with the NOISE branch compiled in and never taken, the second table uploaded
    eta1               eta = 1: Philox + Box-Muller per four elements inside every inner step
For each: the median ms per call and images/s, and from profiled calls of their own the time of the `update` kernel class per launch (median over
--profile-iters calls, with the spread of those calls).  There is no target: the step kernel is stream-bound, and this reports what the noise costs.
Image quality is NOT evaluated: the weights are synthetic.
    python tools/stochastic_bench.py [--images N] [--iters 5] [--profile-iters 5] [--json out.json]"""
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
ap.add_argument("--images", type=int, default=64)
ap.add_argument("--n-iter", type=int, default=35)
ap.add_argument("--guidance", type=float, default=6.0)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--profile-iters", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
S, B = 32, args.images
dev = torch.device("cuda", 0)
cfg = config_100m(S)
m = Denoiser(**asdict(cfg)).to(dev)
m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 5).items()})
m.reserve(2 * B)
gen = DiffusionGenerator(m, None, dev, torch.float32)
rng = torch.Generator().manual_seed(11)
eps = torch.randn(B, 4, S, S, generator=rng).to(dev)
labels = (torch.randn(B, 768, generator=rng) * 0.5).to(dev)
kw = dict(n_iter=args.n_iter, class_guidance=args.guidance, seeds=eps, img_size=S, sharp_f=0.0, bright_f=0.0, exponent=1)
coeffs = schedule.step_coefficients(schedule.noise_schedule(args.n_iter, 1))
n = coeffs.shape[0]
keys = [schedule.noise_key(11, b) for b in range(B)]

RUNS = {
    "generate_latents": lambda: gen.generate_latents(labels, num_imgs=B, **kw),
    "eta0_new_entry": lambda: m.sample_latents_requests(eps, labels, [coeffs] * B, [args.guidance] * B, noise_coeffs=[np.zeros(n, np.float32)] * B,
                                                        noise_keys=keys),
    "eta1": lambda: gen.generate_latents(labels, num_imgs=B, eta=1.0, noise_seeds=keys, **kw),
}
res = {"config": "C1 100M 256px", "images": B, "n_levels": n, "guidance": args.guidance, "iters": args.iters, "profile_iters": args.profile_iters}
outs = {}
for name, run in RUNS.items():
    outs[name] = run(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    per = []
    m.set_profile(["update"])
    try:
        for _ in range(args.profile_iters):
            run(); torch.cuda.synchronize()
            ms, launches = m.get_profile("update")
            assert launches == n, (launches, n)
            per.append(ms / launches * 1e3)
            m.set_profile(["update"])            # (a new accumulation per call)
    finally:
        m.set_profile([])
    res[name] = {"ms": round(t * 1e3, 2), "images_per_s": round(B / t, 2), "ms_all": [round(v * 1e3, 2) for v in ts],
                 "update_us_per_launch": round(sorted(per)[len(per) // 2], 3), "update_us_all": [round(v, 3) for v in per]}
    print(f"{name:18s} {t * 1e3:8.1f} ms per call, {B / t:7.2f} images/s; update {res[name]['update_us_per_launch']:.2f} us per launch "
          f"(calls: {min(per):.2f} .. {max(per):.2f})")
base = res["generate_latents"]
spread = max(base["update_us_all"]) - min(base["update_us_all"])
for name in ("eta0_new_entry", "eta1"):
    res[name]["time_ratio"] = round(res[name]["ms"] / base["ms"], 4)
    res[name]["update_us_over_deterministic"] = round(res[name]["update_us_per_launch"] - base["update_us_per_launch"], 3)
    print(f"{name} / generate_latents: time {res[name]['time_ratio']:.4f} x; update per launch {res[name]['update_us_over_deterministic']:+.2f} us "
          f"(call-to-call spread of the deterministic arm {spread:.2f} us)")
res["deterministic_update_spread_us"] = round(spread, 3)
res["eta0_bitwise_equal_generate_latents"] = bool(torch.equal(outs["eta0_new_entry"], outs["generate_latents"]))
res["eta1_differs"] = bool(not torch.equal(outs["eta1"], outs["generate_latents"]))
print("eta0_new_entry bitwise equal to generate_latents:", res["eta0_bitwise_equal_generate_latents"], "; eta1 differs:", res["eta1_differs"])
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""The shaped guidance update beside plain CFG, at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents, 64 images, 35 steps, guidance 6) in one
process, at the sampler level (no text encoder, no VAE).  Four arms, the same start noise and labels:
    generate_latents   tld_sample, the yardstick
    neutral_new_entry  the same trajectory through tld_sample_requests_shaped with neutral rows: the third table uploaded, and since no request is
                       shaped at any step, no statistics launch and the NOISE flavour of the step (on zeros) instead of the SHAPE one
    rescale            guidance_rescale = 0.7: one statistics launch (one workgroup per image) before every step
    apg_momentum       apg_eta = 0, apg_norm = 2.5, apg_momentum = -0.5 with guidance_rescale = 0.7: the same launch reading the momentum buffer, the step
                       reading and writing it
For each: the median ms per call and images/s, and from profiled calls of their own the time of the `update` kernel class per STEP (the step launch
plus, where there is one, the statistics launch; median over --profile-iters calls, with the spread of those calls).  There is no target: this
reports what the shape costs.  Image quality is NOT evaluated: the weights are synthetic.
    python tools/guidance_shape_bench.py [--images N] [--iters 5] [--profile-iters 5] [--json out.json]"""
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

# arm -> (call, `update` launches per call)
RUNS = {
    "generate_latents": (lambda: gen.generate_latents(labels, num_imgs=B, **kw), n),
    "neutral_new_entry": (lambda: m.sample_latents_requests(eps, labels, [coeffs] * B, [args.guidance] * B,
                                                            shape=[schedule.GUIDANCE_SHAPE_NEUTRAL] * B), n),
    "rescale": (lambda: gen.generate_latents(labels, num_imgs=B, guidance_rescale=0.7, **kw), 2 * n),
    "apg_momentum": (lambda: gen.generate_latents(labels, num_imgs=B, guidance_rescale=0.7, apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5, **kw), 2 * n),
}
res = {"config": "C1 100M 256px", "images": B, "n_levels": n, "guidance": args.guidance, "iters": args.iters, "profile_iters": args.profile_iters}
outs = {}
for name, (run, want_launches) in RUNS.items():
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
            assert launches == want_launches, (name, launches, want_launches)
            per.append(ms / n * 1e3)
            m.set_profile(["update"])            # (a new accumulation per call)
    finally:
        m.set_profile([])
    res[name] = {"ms": round(t * 1e3, 2), "images_per_s": round(B / t, 2), "ms_all": [round(v * 1e3, 2) for v in ts], "update_launches": want_launches,
                 "update_us_per_step": round(sorted(per)[len(per) // 2], 3), "update_us_all": [round(v, 3) for v in per]}
    print(f"{name:18s} {t * 1e3:8.1f} ms per call, {B / t:7.2f} images/s; update {res[name]['update_us_per_step']:.2f} us per step in "
          f"{want_launches // n} launch(es) (calls: {min(per):.2f} .. {max(per):.2f})")
base = res["generate_latents"]
spread = max(base["update_us_all"]) - min(base["update_us_all"])
for name in ("neutral_new_entry", "rescale", "apg_momentum"):
    res[name]["time_ratio"] = round(res[name]["ms"] / base["ms"], 4)
    res[name]["update_us_over_plain"] = round(res[name]["update_us_per_step"] - base["update_us_per_step"], 3)
    print(f"{name} / generate_latents: time {res[name]['time_ratio']:.4f} x; update per step {res[name]['update_us_over_plain']:+.2f} us "
          f"(call-to-call spread of the plain arm {spread:.2f} us)")
res["plain_update_spread_us"] = round(spread, 3)
res["neutral_inside_plain_spread"] = bool(abs(res["neutral_new_entry"]["update_us_over_plain"]) <= spread)
res["neutral_bitwise_equal_generate_latents"] = bool(torch.equal(outs["neutral_new_entry"], outs["generate_latents"]))
res["shaped_differ"] = bool(not torch.equal(outs["rescale"], outs["generate_latents"]) and not torch.equal(outs["apg_momentum"], outs["rescale"]))
print("neutral_new_entry bitwise equal to generate_latents:", res["neutral_bitwise_equal_generate_latents"], "; inside the plain arm's spread:",
      res["neutral_inside_plain_spread"], "; the shaped arms differ:", res["shaped_differ"])
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""Per-step guidance beside the CFG-doubled call, at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents, 64 images, 35 steps, guidance 6) in
one process, at the sampler level (no text encoder, no VAE); ``--image-size 64`` is C3 (512 px, 16 images).  Four arms, the same noise and labels:
    generate_latents   tld_sample, the yardstick: 2 x B x n_levels model-sample forwards
    full_table         generate_latents_requests with a table that guides every forward (tld_sample_requests_guided): the same
                       forwards through the per-step row tables and the slot lookup
    middle_half        an interval that guides the middle half of the levels: the conditional prediction alone outside it
    guidance_one       g = 1 throughout: no unconditional sample at all
For each: the median ms per call, images/s, the (cond, uncond) model samples the engine enqueued (Denoiser.sample_rows) beside the forwards of a
CFG-doubled call, and their ratio; one JSON line at the end.  Image quality under an interval is NOT evaluated: the weights are synthetic.
    python tools/guidance_interval_bench.py [--image-size 64] [--images N] [--iters 5] [--json out.json]"""
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
ap.add_argument("--image-size", type=int, default=32, choices=(32, 64), help="latent side: 32 = C1 (256 px), 64 = C3 (512 px)")
ap.add_argument("--images", type=int, default=None, help="images per call (default 64 at C1, 16 at C3)")
ap.add_argument("--n-iter", type=int, default=35)
ap.add_argument("--guidance", type=float, default=6.0)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
S = args.image_size
B = args.images if args.images is not None else (64 if S == 32 else 16)
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
sig = coeffs[:, 0]
lo_i, hi_i = n // 4, n // 4 + n // 2 - 1                          # the middle half of the levels, by index
middle = (float(sig[hi_i]), float(sig[lo_i]))
tab_mid = schedule.guidance_table(coeffs, args.guidance, middle)
assert int((tab_mid != 1.0).sum()) == n // 2

RUNS = {
    "generate_latents": lambda: gen.generate_latents(labels, num_imgs=B, **kw),
    "full_table": lambda: gen.generate_latents_requests(labels, guidance_schedule=[np.full(n, args.guidance, np.float32)] * B, **kw),
    "middle_half": lambda: gen.generate_latents_requests(labels, guidance_interval=middle, **kw),
    "guidance_one": lambda: gen.generate_latents_requests(labels, guidance_schedule=[np.ones(n, np.float32)] * B, **kw),
}
doubled = 2 * B * n
res = {"config": f"{'C1' if S == 32 else 'C3'} 100M {8 * S}px", "images": B, "n_levels": n, "guidance": args.guidance, "interval": middle,
       "iters": args.iters, "cfg_doubled_forwards": doubled}
outs = {}
for name, run in RUNS.items():
    outs[name] = run(); torch.cuda.synchronize()
    rows = m.sample_rows()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    res[name] = {"ms": round(t * 1e3, 2), "images_per_s": round(B / t, 2), "cond_rows": rows[0], "uncond_rows": rows[1],
                 "row_ratio": round(sum(rows) / doubled, 4), "ms_all": [round(v * 1e3, 2) for v in ts]}
    print(f"{name:18s} {t * 1e3:8.1f} ms per call, {B / t:7.2f} images/s, model samples cond {rows[0]} + uncond {rows[1]} of {doubled} "
          f"(ratio {sum(rows) / doubled:.3f})")
base = res["generate_latents"]["ms"]
for name in ("full_table", "middle_half", "guidance_one"):
    res[name]["time_ratio"] = round(res[name]["ms"] / base, 4)
    print(f"{name} / generate_latents: time {res[name]['time_ratio']:.3f} x, rows {res[name]['row_ratio']:.3f} x")
res["full_table_bitwise_equal_generate_latents"] = bool(torch.equal(outs["full_table"], outs["generate_latents"]))
print("full_table bitwise equal to generate_latents:", res["full_table_bitwise_equal_generate_latents"])
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

#!/usr/bin/env python3
"""One mixed sampler call beside the grouped calls it replaces, at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents), in one process,
at the sampler level (no text encoder, no VAE: both ways share them).  64 requests in four groups of 16 with (guidance, n_iter) =
(3, 15), (6, 15), (6, 35), (4.5, 25):
    grouped    what RequestBatcher(mixed=False) makes of them: four generate_latents calls of 16 (the existing code, the yardstick)
    mixed      one generate_latents_requests call of 64 (tld_sample_requests)
and two side cases:
    uniform    generate_latents_requests with 64 identical requests (35 levels, guidance 6) beside generate_latents of the same batch
    eight      eight requests with eight guidance values (35 levels) in one call beside eight one-image generate_latents calls
Reports the median ms of each, ms per step, the `update` class time per launch (HIP events, Denoiser.get_profile) and the number of
model-sample forwards, 2 x sum(n_levels) either way; one JSON line at the end.
    python tools/mixed_batch_bench.py [--iters 5] [--json out.json]"""
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
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = config_100m(32)
m = Denoiser(**asdict(cfg)).to(dev)
m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 5).items()})
m.reserve(128)
gen = DiffusionGenerator(m, None, dev, torch.float32)
S = 32
rng = torch.Generator().manual_seed(11)
eps = torch.randn(64, 4, S, S, generator=rng).to(dev)
labels = (torch.randn(64, 768, generator=rng) * 0.5).to(dev)
GROUPS = [(3.0, 15), (6.0, 15), (6.0, 35), (4.5, 25)]
guid = [g for g, _ in GROUPS for _ in range(16)]
n_it = [n for _, n in GROUPS for _ in range(16)]
kw = dict(sharp_f=0.0, bright_f=0.0, exponent=1)


def grouped():
    return torch.cat([gen.generate_latents(labels[16 * k:16 * k + 16], n_iter=n, num_imgs=16, class_guidance=g, img_size=S, seeds=eps[16 * k:16 * k + 16], **kw)
                      for k, (g, n) in enumerate(GROUPS)])


def mixed():
    return gen.generate_latents_requests(labels, n_iter=n_it, class_guidance=guid, seeds=eps, **kw)


def uniform_old():
    return gen.generate_latents(labels, n_iter=35, num_imgs=64, class_guidance=6, img_size=S, seeds=eps, **kw)


def uniform_new():
    return gen.generate_latents_requests(labels, n_iter=35, class_guidance=6, seeds=eps, **kw)


G8 = [1.5, 2.0, 3.0, 4.0, 4.5, 6.0, 7.5, 9.0]


def eight_calls():
    return torch.cat([gen.generate_latents(labels[b:b + 1], n_iter=35, num_imgs=1, class_guidance=G8[b], img_size=S, seeds=eps[b:b + 1], **kw) for b in range(8)])


def eight_mixed():
    return gen.generate_latents_requests(labels[:8], n_iter=35, class_guidance=G8, seeds=eps[:8], **kw)


levels = [len(schedule.noise_schedule(n, 1)) for n in n_it]
counts = sorted(levels, reverse=True)
RUNS = {   # name: (callable, sampler steps = update launches, model-sample forwards)
    "grouped": (grouped, sum(len(schedule.noise_schedule(n, 1)) for _, n in GROUPS), 2 * sum(levels)),
    "mixed": (mixed, counts[0], 2 * sum(schedule.active_prefix(counts))),
    "uniform_generate_latents": (uniform_old, 35, 2 * 64 * 35),
    "uniform_requests": (uniform_new, 35, 2 * 64 * 35),
    "eight_one_image_calls": (eight_calls, 8 * 35, 2 * 8 * 35),
    "eight_mixed": (eight_mixed, 35, 2 * 8 * 35),
}
res = {"config": "C1 100M 256px", "groups": GROUPS, "iters": args.iters}
outs = {}
for name, (run, steps, forwards) in RUNS.items():
    outs[name] = run(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); run(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t = sorted(ts)[len(ts) // 2]
    m.reserve_profile("update", steps)
    m.set_profile(["update"]); run(); ms, n = m.get_profile("update"); m.set_profile(())
    assert n == steps, (name, n, steps)
    res[name] = {"ms": round(t * 1e3, 2), "steps": steps, "ms_per_step": round(t * 1e3 / steps, 3), "update_us_per_launch": round(ms / n * 1e3, 2),
                 "model_sample_forwards": forwards, "ms_all": [round(v * 1e3, 2) for v in ts]}
    print(f"{name:26s} {t * 1e3:8.1f} ms, {steps} steps ({t * 1e3 / steps:.3f} ms per step), update class {ms / n * 1e3:.1f} us per launch x {n}, "
          f"{forwards} model-sample forwards")
assert RUNS["grouped"][2] == RUNS["mixed"][2]
for a, b in (("grouped", "mixed"), ("uniform_generate_latents", "uniform_requests"), ("eight_one_image_calls", "eight_mixed")):
    res[f"{b}_bitwise_equal_{a}"] = bool(torch.equal(outs[a], outs[b]))
    res[f"{b}_over_{a}"] = round(res[b]["ms"] / res[a]["ms"], 4)
    print(f"{b} / {a}: {res[f'{b}_over_{a}']:.3f} x, results bitwise equal: {res[f'{b}_bitwise_equal_{a}']}")
line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

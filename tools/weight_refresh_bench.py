#!/usr/bin/env python3
"""Cost of bringing an inference engine up to date with a live Trainer's EMA weights, at the C1 model (100 M parameters,
max_batch 128), in one process:

  (a) a fresh load, the only way before the device refresh:    den.load_state_dict(tr.ema_state_dict()); den.reserve(128)
      -- a device-to-host copy of the vector and an engine rebuild (upload + the refresh kernels).  Wall time, ending in a synchronise.
  (b) the device path:                                          den.load_flat(tr.ema)
      -- one device-to-device copy and the refresh kernels, in place.  Wall time ending in a synchronise, and device time from HIP events.

tools/weight_refresh_bench.py [--batch 128] [--layers 12] [--reps-host 2] [--reps-device 20] [--out profiles/weight_refresh_bench.txt]
Prints the figures and writes them to --out.  No test asserts a time: a record."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_latent_diffusion_amd import TrainConfig, Trainer, config_100m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--reps-host", type=int, default=2)
ap.add_argument("--reps-device", type=int, default=20)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "weight_refresh_bench.txt"))
args = ap.parse_args()

dev = torch.device("cuda", 0)
cfg = config_100m(32)
cfg.n_layers = args.layers
tr = Trainer(cfg, TrainConfig(batch_size=8), device=dev, init_seed=5, max_batch=8)       # (the trainer only supplies the vectors: a small batch)
g = torch.Generator().manual_seed(1)
tr.train_step(torch.randn(8, 4, 32, 32, generator=g) * 0.8, torch.randn(8, 768, generator=g) * 0.5)      # params != ema
den = tr.make_denoiser(args.batch)
x = torch.randn(4, 4, 32, 32, generator=g).to(dev)
sigma, lab = torch.full((4, 1), 0.5, device=dev), (torch.randn(4, 768, generator=g) * 0.5).to(dev)
den(x, sigma, lab)
torch.cuda.synchronize()

host = []
for _ in range(args.reps_host):
    t0 = time.perf_counter()
    den.load_state_dict(tr.ema_state_dict())
    den.reserve(args.batch)
    torch.cuda.synchronize()
    host.append((time.perf_counter() - t0) * 1e3)
ref = den(x, sigma, lab).clone()

den.load_flat(tr.params)                         # other weights in between, and the first (allocating) call outside the timed ones
assert not torch.equal(den(x, sigma, lab), ref)
wall, devt = [], []
for _ in range(args.reps_device):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    den.load_flat(tr.ema)
    b.record()
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
    devt.append(a.elapsed_time(b))
same = torch.equal(den(x, sigma, lab), ref)

n = tr.numel
med = lambda v: sorted(v)[len(v) // 2]
lines = [
    "Bringing an inference engine (100 M model, d = 768, %d blocks, 256 tokens, max_batch %d) up to date with a Trainer's EMA weights," % (args.layers, args.batch),
    "one MI355X, one process (tools/weight_refresh_bench.py).  %d parameters = %.1f MB as fp32.  Not gated anywhere: a record." % (n, n * 4 / 1e6),
    "",
    "(a) fresh load  den.load_state_dict(tr.ema_state_dict()); den.reserve(%d)   wall ms, synchronised:   %s" % (args.batch, "  ".join("%.1f" % v for v in host)),
    "(b) device path den.load_flat(tr.ema)                                        wall ms, synchronised:   median %.3f  (min %.3f, max %.3f; %d calls)"
    % (med(wall), min(wall), max(wall), len(wall)),
    "                (the private device-to-device copy of the vector + 4 kernels) device ms, HIP events:   median %.3f  (min %.3f, max %.3f)"
    % (med(devt), min(devt), max(devt)),
    "forward after (b) equals forward after (a), bit for bit: %s" % same,
]
text = "\n".join(lines) + "\n"
print(text, end="")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write(text)
if not same:
    sys.exit(1)

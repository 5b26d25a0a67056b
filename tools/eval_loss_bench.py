#!/usr/bin/env python3
"""Time the held-out loss (Trainer.eval_loss) beside the training step, in one process: 100 M-parameter denoiser, 32x32x4
latents, batch 128, a device-resident dataset of uint8 codes.  Per held-out batch (one tld_train_prepare_batch_at + tld_train_forward_loss +
tld_train_loss_buckets): with the model's own weights, and with the EMA weights -- which includes both operand rebuilds, from the EMA vector at the
start of every call and from the bound parameters when training goes on.  Prints one JSON line.
tools/eval_loss_bench.py [--batch 128] [--batches 16] [--steps 20] [--warmup 5] [--image-size 32] [--layers 12]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_latent_diffusion_amd import DeviceLatentDataset, TrainConfig, Trainer, config_100m, quantize_latents  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--batches", type=int, default=16, help="held-out batches per eval_loss call")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--image-size", type=int, default=32)
ap.add_argument("--layers", type=int, default=12)
args = ap.parse_args()

dev = torch.device("cuda", 0)
S = args.image_size
cfg = config_100m(S)
cfg.n_layers = args.layers
tr = Trainer(cfg, TrainConfig(batch_size=args.batch), device=dev, init_seed=5, max_batch=args.batch, loss_buckets=None)
rows = args.batches * args.batch
g = torch.Generator().manual_seed(2)
ds = DeviceLatentDataset(quantize_latents(torch.randn(rows, 4, S, S, generator=g) * 0.8 * 8), (torch.randn(rows, 768, generator=g) * 0.5).half(), device=dev)
idx = [b for b in ds.batches(args.batch, seed=0, epoch=0) if len(b) == args.batch]
held_out = torch.arange(rows, device=dev)


def timed(fn, n, warmup):
    """(wall ms per call, median HIP-event ms per call) of fn(i)"""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    t0 = time.perf_counter()
    for i in range(n):
        ev[i].record()
        fn(warmup + i)
    ev[n].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / n * 1e3
    each = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(n))
    return wall, each[len(each) // 2]


step = timed(lambda i: tr.train_step_from(ds, idx[i % len(idx)]), args.steps, args.warmup)
results = {}
for weights in ("model", "ema"):
    out = {}
    wall, med = timed(lambda i: out.__setitem__("res", tr.eval_loss(ds, held_out, weights=weights)), 5, 2)
    results[weights] = {"ms_per_eval": wall, "ms_per_batch": wall / args.batches, "ms_per_batch_median_events": med / args.batches, **out["res"].cpu()}
    results[weights]["bucket_loss"] = [float(v) for v in results[weights]["bucket_loss"]]
    results[weights]["bucket_count"] = [int(v) for v in results[weights]["bucket_count"]]
# one held-out batch on the EMA weights between two training steps: both operand rebuilds are inside the interval
one = timed(lambda i: (tr.eval_loss(ds, held_out[:args.batch], weights="ema"), tr.train_step_from(ds, idx[i % len(idx)])), args.steps, 2)
step_after = timed(lambda i: tr.train_step_from(ds, idx[i % len(idx)]), args.steps, 2)
print(json.dumps({"metric": f"held-out loss per batch beside the training step (100M denoiser, {S}x{S}x4 latents, batch {args.batch})", "unit": "ms",
                  "graph": tr.use_graph, "cpu_threads": torch.get_num_threads(), "batches_per_eval": args.batches,
                  "train_step": {"ms_per_step": step[0], "ms_per_step_median_events": step[1]},
                  "train_step_after_the_evaluations": {"ms_per_step": step_after[0], "ms_per_step_median_events": step_after[1]},
                  "eval_model_weights": results["model"], "eval_ema_weights": results["ema"],
                  "one_ema_batch_plus_one_step": {"ms": one[0], "ms_median_events": one[1], "minus_the_step": one[1] - step_after[1]},
                  "forward_over_step": results["model"]["ms_per_batch_median_events"] / step[1]}))

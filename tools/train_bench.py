#!/usr/bin/env python3
"""Time the native training step (tld/train.py:118-175): 100 M-parameter denoiser, 32x32x4 latents, the reference's
TrainConfig (batch 128, Adam lr 3e-4, EMA 0.999).  One step = make_batch (host RNG, as the reference) + forward + backward + Adam + EMA.
Prints one JSON line in bench.py's vocabulary.   tools/train_bench.py [--batch 128] [--steps 10] [--warmup 2] [--layers 12] [--image-size 32]
[--patch-size 2] [--no-cpu-baseline] [--max-grad-norm X] [--skip-nonfinite]   (the last two: the guarded optimizer step, to time beside the plain one;
--image-size: the latent side, e.g. 48 = 576 tokens, the 384 px fine-tuning grid; the TFLOP/s figures
are quoted at the default 32 only, where the op count below applies)
--weight-decay W / --freeze GLOB (repeatable) / --lr-warmup N: the grouped optimizer step (AdamW with the usual no-decay exemptions, frozen tensors, a
warm-up on the applied steps: DESIGN.md section 7.3); every run also reports the optimizer part alone in HIP-event time ("optimizer_ms_events")
--device-data [--latent-dtype uint8|float16|float32]: the same model and batch size through train_step (host make_batch + pinned staging) and through
train_step_from (a device-resident dataset, one preparation kernel: DESIGN.md section 7.11) in one process; one JSON line with both."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_latent_diffusion_amd import TrainConfig, Trainer, config_100m  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=128)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--layers", type=int, default=12)
ap.add_argument("--image-size", type=int, default=32)
ap.add_argument("--patch-size", type=int, default=2)
ap.add_argument("--no-cpu-baseline", action="store_true")
ap.add_argument("--max-grad-norm", type=float, default=None)
ap.add_argument("--skip-nonfinite", action="store_true")
ap.add_argument("--weight-decay", type=float, default=0.0)
ap.add_argument("--freeze", action="append", default=[])
ap.add_argument("--lr-warmup", type=int, default=0)
ap.add_argument("--device-data", action="store_true")
ap.add_argument("--latent-dtype", choices=("uint8", "float16", "float32"), default="uint8")
args = ap.parse_args()

dev = torch.device("cuda", 0)
S = args.image_size
cfg = config_100m(S)
cfg.patch_size = args.patch_size
cfg.n_layers = args.layers
tc = TrainConfig(batch_size=args.batch)
grouped = {}
if args.weight_decay or args.freeze or args.lr_warmup:
    from transformer_latent_diffusion_amd import opt_groups, param_layout
    specs = [dict(match=args.freeze, frozen=True)] if args.freeze else []
    grouped = dict(weight_decay=args.weight_decay, param_groups=specs + (opt_groups.no_decay(param_layout(cfg)) if args.weight_decay else []))
    if args.lr_warmup:
        grouped.update(lr_schedule=opt_groups.warmup_constant(args.lr_warmup), schedule_steps=args.lr_warmup)
tr = Trainer(cfg, tc, device=dev, init_seed=5, max_batch=args.batch, max_grad_norm=args.max_grad_norm, skip_nonfinite=args.skip_nonfinite, **grouped)
g = torch.Generator().manual_seed(1)
x = torch.randn(args.batch, 4, S, S, generator=g) * 0.8
y = torch.randn(args.batch, 768, generator=g) * 0.5
rng, tg = np.random.default_rng(0), torch.Generator().manual_seed(0)


def timed_steps(step_fn):
    """warmup + steps calls of step_fn(i): (wall ms per step, median HIP-event ms per step, last loss)."""
    for i in range(args.warmup):
        step_fn(i)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t_start = time.perf_counter()
    for i in range(args.steps):
        ev[i].record()
        out = step_fn(args.warmup + i)
    ev[args.steps].record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t_start) / args.steps * 1e3
    each = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(args.steps))
    return wall, each[len(each) // 2], float(out)


if args.device_data:
    from transformer_latent_diffusion_amd import DeviceLatentDataset, quantize_latents
    rows = 16 * args.batch
    gd = torch.Generator().manual_seed(2)
    lat = torch.randn(rows, 4, S, S, generator=gd) * 0.8 * 8             # unscaled latents, as the reference stores them
    lat = {"uint8": quantize_latents, "float16": lambda t: t.half(), "float32": lambda t: t}[args.latent_dtype](lat)
    ds = DeviceLatentDataset(lat, (torch.randn(rows, 768, generator=gd) * 0.5).half(), device=dev)
    idx = [b for b in ds.batches(args.batch, seed=0, epoch=0) if len(b) == args.batch]
    # the host path: what the loader would hand over (fp32 latents / scale, fp32 embeddings) -> make_batch on the host -> pinned staging
    t_h = time.perf_counter()
    for _ in range(5):
        tr.make_batch(x, y, rng, tg)
    host_prepare_ms = (time.perf_counter() - t_h) / 5 * 1e3
    host = timed_steps(lambda i: tr.train_step(x, y, rng, tg))
    device = timed_steps(lambda i: tr.train_step_from(ds, idx[i % len(idx)]))
    # the preparation kernel alone, HIP events around single launches; a matrix product is queued first so that the host has enqueued the launch and
    # both events before the device reaches them (otherwise the interval is the host's launch path, not the kernel)
    times, w = [], torch.randn(4096, 4096, device=dev)
    for i in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w @ w
        a.record(); tr.prepare_batch(ds, idx[i % len(idx)]); b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    kernel_ms = sorted(times[5:])[len(times[5:]) // 2]
    E = 4 * S * S
    nbytes = args.batch * (E * ds.latents.element_size() + 768 * 2 + 8 + 2 * E * 4 + 768 * 4 + 4)
    side = lambda t, extra: dict({"ms_per_step": t[0], "ms_per_step_median_events": t[1], "samples_per_s": args.batch / t[0] * 1e3, "loss": t[2]}, **extra)
    print(json.dumps({"metric": f"training step, host batch against device batch (100M denoiser, {S}x{S}x4 latents, batch {args.batch})", "unit": "ms/step",
                      "steps": args.steps, "warmup": args.warmup, "cpu_threads": torch.get_num_threads(), "graph": tr.use_graph,
                      "host_data": side(host, {"path": "train_step: make_batch on the host, pinned staging, 4 copies", "make_batch_host_ms": host_prepare_ms}),
                      "device_data": side(device, {"path": f"train_step_from: resident {args.latent_dtype} latents + fp16 embeddings, one kernel",
                                                   "prepare_kernel_ms": kernel_ms, "prepare_bytes": nbytes, "prepare_GB_per_s": nbytes / kernel_ms / 1e6}),
                      "device_over_host": device[0] / host[0]}))
    sys.exit(0)

# device-resident batch (the loader's job); the per-step host work of tld/train.py:118-138 (Beta draw, randn, mask) is timed with the step
for _ in range(args.warmup):
    loss = tr.train_step(x, y, rng, tg)
torch.cuda.synchronize()
marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
t0 = time.perf_counter()
for i in range(args.steps):
    marks[i].record()
    loss = tr.train_step(x, y, rng, tg)
marks[args.steps].record()
torch.cuda.synchronize()
dt = time.perf_counter() - t0
ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
# the device part alone (batch prepared once): forward_backward + optimizer_step
xn, nl, lab = tr.make_batch(x, y, rng, tg)
xn, nl, lab, xd = xn.to(dev), nl.to(dev), lab.to(dev), x.to(dev)
for _ in range(2):
    tr.forward_backward(xn, nl, lab, xd); tr.optimizer_step()
torch.cuda.synchronize()
t1 = time.perf_counter()
for _ in range(args.steps):
    tr.forward_backward(xn, nl, lab, xd); tr.optimizer_step()
torch.cuda.synchronize()
ddt = (time.perf_counter() - t1) / args.steps
fwd_gflop = 46.163 * args.layers / 12.0            # per sample (the 15.5 MFLOP of embed / out / cond are in the noise)
step_tflop = 3.0 * fwd_gflop * args.batch / 1e3     # forward + backward (2x) by the reference's op count
ntok = (S // args.patch_size) ** 2
line = {"metric": f"training samples/sec (100M denoiser, {S}x{S}x4 latents, fwd + bwd + Adam + EMA)", "value": args.batch * args.steps / dt, "unit": "samples/s",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "ms_per_step_median": ms[len(ms) // 2],
        "ms_per_step_device_only": ddt * 1e3, "higher_is_better": True, "dtype": "bf16 operands / fp32 master", "data": "synthetic",
        "config": {"workload": f"training step, 100M-param denoiser (d=768, L={args.layers}, {ntok} tokens), batch {args.batch}, Adam lr 3e-4, EMA 0.999"},
        "loss": float(loss), "algorithmic_tflops": step_tflop / ddt, "frac_of_bf16_mfma_peak": step_tflop / ddt / 2500.0,
        "roofline": {"bound": "mfma", "achieved": step_tflop / ddt, "peak": 2500.0, "unit": "TFLOP/s", "frac": step_tflop / ddt / 2500.0,
                     "note": "whole step (3 x the reference forward op count) over the device-only step time; per-kernel times: profiles/r05_train_kernel_stats.csv (rocprofv3 --kernel-trace --stats of this tool)"}}
# the optimizer part alone on the last step's gradients, HIP events around single calls; a matrix product is queued first so that the host has
# enqueued the launches and both events before the device reaches them
opt_times, wm = [], torch.randn(4096, 4096, device=dev)
for i in range(25):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    wm @ wm
    a.record(); tr.optimizer_step(); b.record()
    b.synchronize()
    opt_times.append(a.elapsed_time(b))
line["optimizer_ms_events"] = sorted(opt_times[5:])[len(opt_times[5:]) // 2]
if getattr(tr, "grouped", False):
    frozen = sum(n for n, q in zip(tr._seg_numel, tr._seg_group) if tr._groups[q][2])
    line["optimizer_groups"] = {"weight_decay": args.weight_decay, "freeze": args.freeze, "lr_warmup": args.lr_warmup, "groups": len(tr._groups),
                                "frozen_fraction": frozen / tr.numel}
if tr.guarded or getattr(tr, "grouped", False):
    line["optimizer_guard"] = dict(tr.optimizer_stats(), max_grad_norm=args.max_grad_norm, skip_nonfinite=args.skip_nonfinite)
if not args.no_cpu_baseline:
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    sd = synth_state_dict(cfg, 5)
    nb = 4
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    t2 = time.perf_counter()
    train_step_reference(cfg, sd, x[:nb], torch.tensor(rng.beta(1, 2.5, nb)), torch.randn(nb, 4, S, S), y[:nb], torch.zeros(nb, dtype=torch.bool))
    cdt = time.perf_counter() - t2
    line["cpu_baseline"] = {"value": nb / cdt, "unit": "samples/s", "cores": torch.get_num_threads(), "kind": "port",
                            "sample": f"forward + autograd backward of {nb} samples on the fp32 torch restatement (oracle/torch_ref.py), no optimizer"}
if (S, args.patch_size) != (32, 2):
    for k in ("algorithmic_tflops", "frac_of_bf16_mfma_peak", "roofline"):
        line.pop(k)
print(json.dumps(line))

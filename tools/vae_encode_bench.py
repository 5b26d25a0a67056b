#!/usr/bin/env python
"""VAE encode (tld/data.py: images -> latents) on one GPU: images/s and per-kernel-class HIP-event times of the native encoder at the
SDXL-VAE geometry -- 256 px at batch 16 and 64, and 512 px by default.

    python tools/vae_encode_bench.py [--batches 16,64] [--size 256] [--big-size 512] [--big-batch 16] [--iters 5]

Prints one JSON line.  FLOPs are the algorithmic ones of the module graph (convolutions, attention, 1x1 shortcuts, quant_conv), counted
from the state-dict spec (vae_encoder_spec)."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from transformer_latent_diffusion_amd.vae_encoder import AutoencoderKLEncoder, VaeEncoderConfig, vae_encoder_spec  # noqa: E402

PEAK_TFLOPS = 2500.0        # dense bf16 MFMA, MI355X


def encode_flops(cfg: VaeEncoderConfig, size: int, only_conv3x3: bool = False) -> float:
    """2 * MACs per image of AutoencoderKL.encode (only_conv3x3: the implicit-GEMM 3x3 convolutions -- every 3x3 conv but the
    3-channel conv_in, downsamplers and conv_out included)."""
    spec = vae_encoder_spec(cfg)
    boc = list(cfg.block_out_channels)

    def conv(key, hh):
        co, ci, k, _ = spec[key + ".weight"]
        if only_conv3x3 and (k != 3 or ci < 64):
            return 0.0
        return 2.0 * hh * hh * co * ci * k * k

    h = size
    fl = conv("encoder.conv_in", h)
    for i in range(len(boc)):
        for j in range(cfg.layers_per_block):
            r = f"encoder.down_blocks.{i}.resnets.{j}"
            fl += conv(r + ".conv1", h) + conv(r + ".conv2", h)
            if r + ".conv_shortcut.weight" in spec:
                fl += conv(r + ".conv_shortcut", h)
        if i != len(boc) - 1:
            h //= 2
            fl += conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", h)
    c = boc[-1]
    for r in ("encoder.mid_block.resnets.0", "encoder.mid_block.resnets.1"):
        fl += conv(r + ".conv1", h) + conv(r + ".conv2", h)
    if cfg.mid_block_add_attention and not only_conv3x3:
        n = h * h
        fl += 4 * 2.0 * n * c * c + 2 * 2.0 * n * n * c
    fl += conv("encoder.conv_out", h)
    if cfg.use_quant_conv:
        fl += conv("quant_conv", h)
    return fl


def run(cfg, dev, size, batch, iters):
    enc = AutoencoderKLEncoder(cfg, max_batch=batch).to(dev)
    enc._weights_loaded = True                 # (synthetic weights on purpose: no warning)
    x = (torch.rand(batch, 3, size, size, generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    m = enc.moments(x)                         # builds the engine, warms up
    enc.moments(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        enc.moments(x)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / iters
    enc.set_profile(True)
    enc.moments(x)
    prof = enc.get_profile()
    enc.set_profile(False)
    fl, cfl = encode_flops(cfg, size), encode_flops(cfg, size, only_conv3x3=True) * batch
    cms, cn = prof["conv3x3"]
    r = {"size": size, "batch": batch, "images_per_sec": batch / dt, "ms_per_batch": dt * 1e3, "gflop_per_image": fl / 1e9,
         "tflops": batch * fl / dt / 1e12, "frac_of_bf16_mfma_peak": batch * fl / dt / (PEAK_TFLOPS * 1e12),
         "classes_ms": {k: round(v[0], 3) for k, v in prof.items()}, "classes_launches": {k: v[1] for k, v in prof.items()},
         "finite": bool(torch.isfinite(m).all())}
    if cms > 0:
        # the implicit-GEMM 3x3 convolutions (gemm256p_kernel<.., CONV>, stride 1 and stride 2), HIP events on the launch stream
        r["conv3x3"] = {"tflops": cfl / (cms * 1e-3) / 1e12, "frac_of_peak": cfl / (cms * 1e-3) / 1e12 / PEAK_TFLOPS, "launches": cn,
                        "flops": cfl, "total_ms": cms}
    del enc
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="16,64")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--big-size", type=int, default=512)
    ap.add_argument("--big-batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=5)
    a = ap.parse_args()
    cfg = VaeEncoderConfig()
    dev = torch.device("cuda:0")
    runs = [run(cfg, dev, a.size, int(b), a.iters) for b in a.batches.split(",")]
    if a.big_size:
        runs.append(run(cfg, dev, a.big_size, a.big_batch, a.iters))
    head = runs[0]
    out = {"metric": f"vae_encode_images_per_sec_{a.size}px", "value": head["images_per_sec"], "unit": "images/s", "batch": head["batch"],
           "dtype": "bf16", "data": "synthetic (random-init weights)", "peak_tflops": PEAK_TFLOPS, "runs": runs}
    print(json.dumps(out))


if __name__ == "__main__":
    main()

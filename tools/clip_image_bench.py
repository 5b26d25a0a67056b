#!/usr/bin/env python
"""CLIP ViT-L/14 image tower on one GPU: images/s of the native encoder (random-init weights) and the attention kernel's share of it.

    python tools/clip_image_bench.py [--batch 16 64] [--iters 10] [--out profiles/clip_image_bench.txt]

Times are HIP events around whole calls.  ``encode_image`` is timed as a whole; the attention class is timed alone by running the tower's
attention kernel (tld_debug_clip_vis_attention) on a qkv buffer of the same shape once per layer.  The engine has no per-class profile hook, so
im2col, the GEMMs and the row kernels are reported together as the remainder.  The op count is B L (2 n 12 W^2 + 4 n^2 W) plus the patch GEMM; the
fraction of peak is against 2.5 PFLOP/s dense bf16 (16 x the 157.3 TFLOP/s fp32 matrix rate)."""
import argparse, ctypes as C, json, os, sys
import torch
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from transformer_latent_diffusion_amd import _lib                                                     # noqa: E402
from transformer_latent_diffusion_amd.clip_image import ClipImageEncoder, ClipVisionConfig            # noqa: E402

PEAK_BF16 = 16 * 157.3e12

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, nargs="+", default=[16, 64])
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None)
a = ap.parse_args()
cfg = ClipVisionConfig()
w, L, n, g = cfg.width, cfg.layers, cfg.tokens, cfg.grid


def timed(fn, iters):
    fn(); fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e-3


lines = []
for B in a.batch:
    enc = ClipImageEncoder(cfg, max_batch=B).to("cuda")
    enc.load_state_dict(enc.state_dict())
    pix = torch.randn(B, 3, cfg.image_size, cfg.image_size, device="cuda")
    dt = timed(lambda: enc.encode_image(pix), a.iters)
    out = enc.encode_image(pix)
    enc._drop_engine()
    qkv = torch.randn(B * n, 3 * w, device="cuda").to(torch.bfloat16)
    att = torch.empty(B * n, w, device="cuda", dtype=torch.bfloat16)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = _lib.lib()

    def layers():
        for _ in range(L):
            _lib.check(lib.tld_debug_clip_vis_attention(C.c_void_p(qkv.data_ptr()), C.c_void_p(att.data_ptr()), B, n, cfg.heads, st), "attention")
    dt_att = timed(layers, a.iters)
    flops = B * L * (2 * n * 12 * w * w + 4 * n * n * w) + B * g * g * 2 * w * 3 * cfg.patch_size ** 2
    att_flops = B * L * 4 * n * n * w
    lines.append({"metric": "clip_image_images_per_sec", "value": B / dt, "unit": "images/s", "batch": B, "ms_per_batch": dt * 1e3,
                  "gflop_per_image": flops / B / 1e9, "tflops": flops / dt / 1e12, "fraction_of_bf16_peak": flops / dt / PEAK_BF16,
                  "attention_ms_per_batch": dt_att * 1e3, "attention_share": dt_att / dt, "attention_tflops": att_flops / dt_att / 1e12,
                  "gemms_im2col_rows_ms_per_batch": (dt - dt_att) * 1e3, "attention_vs_rest_per_block": dt_att / max(dt - dt_att, 1e-12),
                  "dtype": "bf16 GEMM / attention operands, fp32 residual / LayerNorm / softmax", "data": "synthetic (random-init weights)",
                  "finite": bool(torch.isfinite(out).all())})
    print(json.dumps(lines[-1]))
if a.out:
    with open(a.out, "w") as f:
        f.write("tools/clip_image_bench.py: CLIP ViT-L/14 image tower, HIP-event times (attention timed alone, once per layer)\n")
        for ln in lines:
            f.write(json.dumps(ln) + "\n")

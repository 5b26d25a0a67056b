"""Writes tests/golden/g19_vae_encoder_janus.npz: the VAE ENCODER's downsampler -- and the encoder it is wired into -- computed by an
INDEPENDENT PUBLISHED implementation, HuggingFace ``transformers`` (5.15 in this image) ``models/janus/modeling_janus.py``:

    JanusVQVAEConvDownsample  F.pad(x, (0, 1, 0, 1)) -> conv3x3 stride 2, padding 0          (diffusers Downsample2D with padding = 0)
    JanusVQVAEEncoder         conv_in -> per level num_res_blocks resnets [+ downsample] -> mid (resnet, attention, resnet)
                              -> GroupNorm(32, eps 1e-6) -> swish (in place) -> conv_out (2 latent_channels with double_latent)

That file is the CompVis latent-diffusion encoder (taming-transformers ``Encoder``), from which diffusers' ``AutoencoderKL`` encoder -- the
reference's VAE in tld/data.py -- derives block for block; diffusers itself is absent from this image.  The script loads the SAME synthetic
diffusers-keyed weights (``synth_vae_encoder_state_dict``) into the Janus modules through the key map below and records inputs -> outputs:

* ``ds:*``: the downsampler alone, as published;
* ``enc:*``: the whole ``JanusVQVAEEncoder`` at a tiny geometry ((64, 128), one resnet per level) on one 64-px image: the moments in full,
  every stage (forward hooks) as (mean, rms) plus a fixed strided sample of 8192 values;
* ``sdxl:*``: the SDXL-VAE geometry ((128, 256, 512, 512), two resnets per level: 34 163 592 encoder parameters) on one 64-px image: the
  moments in full, every stage as (mean, rms) plus a fixed strided sample of 2048 values.

ONE deviation from the published constructor, stated here and in the fixture (``deviation``): Janus puts an attention block after every
resnet of its lowest-resolution level (``attn.append`` when ``i_level == num_resolutions - 1``); diffusers' ``DownEncoderBlock2D`` has none,
so that ModuleList is emptied after construction (``len(self.down[i_level].attn) > 0`` in its forward then skips it).  What stays "restated
from the published graph" only: ``quant_conv`` (a 1x1 convolution applied here with ``F.conv2d``) and the diffusers KEY NAMES.
``norm_out`` is taken by a pre-hook of ``conv_out`` with ``.clone()``: Janus applies the swish in place.  Inputs are stored as seeds plus
checksums where the tensor is regenerated with ``torch.Generator`` (CPU) in the test.

    python tools/gen_golden_vae_encoder.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from transformers.models.janus import modeling_janus as mj                                # noqa: E402
from transformers.models.janus.configuration_janus import JanusVQVAEConfig                # noqa: E402

from oracle.gen_golden_vae_blocks import _put, attn_tensors, resnet_tensors               # noqa: E402
from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig, synth_vae_encoder_state_dict   # noqa: E402

DEVIATION = "down[i].attn emptied: diffusers DownEncoderBlock2D has no attention (Janus puts one after every resnet of its lowest level)"


def seeded_image(seed: int, b: int, s: int, scale: float = 0.6) -> torch.Tensor:
    """The fixture's input images: a seeded torch CPU generator, N(0, scale^2) clipped to [-1, 1] (the encoder's input domain)."""
    return (torch.randn(b, 3, s, s, generator=torch.Generator().manual_seed(seed)) * scale).clamp(-1.0, 1.0)


def janus_encoder(cfg: VaeEncoderConfig, sd):
    boc = list(cfg.block_out_channels)
    base = boc[0]
    assert all(c % base == 0 for c in boc) and cfg.norm_num_groups == 32
    jc = JanusVQVAEConfig(in_channels=cfg.in_channels, base_channels=base, channel_multiplier=[c // base for c in boc],
                          num_res_blocks=cfg.layers_per_block, latent_channels=cfg.latent_channels, double_latent=True, dropout=0.0)
    enc = mj.JanusVQVAEEncoder(jc)
    enc.down[len(boc) - 1].attn = torch.nn.ModuleList()          # the one stated deviation
    t = {"conv_in.weight": sd["encoder.conv_in.weight"], "conv_in.bias": sd["encoder.conv_in.bias"],
         "norm_out.weight": sd["encoder.conv_norm_out.weight"], "norm_out.bias": sd["encoder.conv_norm_out.bias"],
         "conv_out.weight": sd["encoder.conv_out.weight"], "conv_out.bias": sd["encoder.conv_out.bias"]}
    for k, v in resnet_tensors(sd, "encoder.mid_block.resnets.0").items():
        t["mid.block_1." + k] = v
    for k, v in attn_tensors(sd, "encoder.mid_block.attentions.0").items():
        t["mid.attn_1." + k] = v
    for k, v in resnet_tensors(sd, "encoder.mid_block.resnets.1").items():
        t["mid.block_2." + k] = v
    for i in range(len(boc)):
        for j in range(cfg.layers_per_block):
            for k, v in resnet_tensors(sd, f"encoder.down_blocks.{i}.resnets.{j}").items():
                t[f"down.{i}.block.{j}.{k}"] = v
        if i != len(boc) - 1:
            t[f"down.{i}.downsample.conv.weight"] = sd[f"encoder.down_blocks.{i}.downsamplers.0.conv.weight"]
            t[f"down.{i}.downsample.conv.bias"] = sd[f"encoder.down_blocks.{i}.downsamplers.0.conv.bias"]
    return _put(enc, **t)


def encode_with_stages(cfg, sd, x):
    """(moments, [(stage name in the engine's vocabulary, tensor)]) from the Janus encoder + quant_conv."""
    enc = janus_encoder(cfg, sd)
    stages = []
    hook = lambda name: (lambda _m, _i, o: stages.append((name, o.detach().clone())))
    enc.conv_in.register_forward_hook(hook("conv_in"))
    for i in range(len(cfg.block_out_channels)):
        for j in range(cfg.layers_per_block):
            enc.down[i].block[j].register_forward_hook(hook(f"down{i}.res{j}"))
        if i != len(cfg.block_out_channels) - 1:
            enc.down[i].downsample.register_forward_hook(hook(f"down{i}.downsample"))
    enc.mid.block_1.register_forward_hook(hook("mid.res0"))
    enc.mid.attn_1.register_forward_hook(hook("mid.attn"))
    enc.mid.block_2.register_forward_hook(hook("mid.res1"))
    enc.conv_out.register_forward_pre_hook(lambda _m, i: stages.append(("norm_out", i[0].detach().clone())))   # after the in-place swish
    with torch.no_grad():
        h = enc(x.clone())
        moments = F.conv2d(h, torch.as_tensor(sd["quant_conv.weight"]), torch.as_tensor(sd["quant_conv.bias"]))
    return moments, stages


def checksum(t: torch.Tensor) -> np.ndarray:
    f = t.double().reshape(-1)
    return np.array([float(f.sum()), float(f.pow(2).sum()), float(f.abs().max())])


def main():
    out = {"transformers_version": np.array(__import__("transformers").__version__), "deviation": np.array(DEVIATION)}
    # ---- 1. the downsampler alone, as published (64 channels, ragged 11 x 14 source) ---------------------------------------------------------------
    cfg = VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1)
    seed = 41
    sd = synth_vae_encoder_state_dict(cfg, seed)
    out["tiny_boc"], out["tiny_layers"], out["tiny_seed"] = np.array(cfg.block_out_channels), np.array(cfg.layers_per_block), np.array(seed)
    with torch.no_grad():
        xd = torch.randn(2, 64, 11, 14, generator=torch.Generator().manual_seed(42)) * 1.2
        ds = _put(mj.JanusVQVAEConvDownsample(64), **{"conv.weight": sd["encoder.down_blocks.0.downsamplers.0.conv.weight"],
                                                     "conv.bias": sd["encoder.down_blocks.0.downsamplers.0.conv.bias"]})
        out["ds:x"] = xd.numpy()
        out["ds:out"] = ds(xd.clone()).numpy()                 # encoder.down_blocks.0.downsamplers.0: [2, 64, 5, 7]
    # ---- 2. the wired encoder, tiny geometry: the moments in full, every stage as (mean, rms) + a strided sample of 8192 values -------------------
    # (the full stages -- 1.3 M values -- are not stored: tests/test_gpu_vae_encoder.py compares every engine stage in full with the restatement,
    # which tests/test_vae_encoder_host.py holds to these samples at 1e-5)
    x = seeded_image(43, 1, 64)
    out["enc:x_seed"], out["enc:x_shape"], out["enc:x_checksum"] = np.array(43), np.array(x.shape), checksum(x)
    moments, stages = encode_with_stages(cfg, sd, x)
    out["enc:moments"] = moments.numpy()
    out["enc:stage_names"] = np.array([n for n, _ in stages])
    for n, t in stages:
        f = t.reshape(-1)
        out["enc:stat:" + n] = np.array([float(f.mean()), float(f.pow(2).mean().sqrt())])
        out["enc:sample:" + n] = f[::max(1, f.numel() // 8192)][:8192].numpy()
    # ---- 3. the wired encoder at the SDXL-VAE geometry, one 64-px image: the moments in full, stages as (mean, rms) + a strided sample --------------
    cfg2, seed2 = VaeEncoderConfig(), 44
    sd2 = synth_vae_encoder_state_dict(cfg2, seed2)
    x2 = seeded_image(45, 1, 64)
    out["sdxl:seed"], out["sdxl:x_seed"], out["sdxl:x_shape"], out["sdxl:x_checksum"] = np.array(seed2), np.array(45), np.array(x2.shape), checksum(x2)
    moments2, stages2 = encode_with_stages(cfg2, sd2, x2)
    out["sdxl:moments"] = moments2.numpy()
    out["sdxl:stage_names"] = np.array([n for n, _ in stages2])
    for n, t in stages2:
        f = t.reshape(-1)
        out["sdxl:stat:" + n] = np.array([float(f.mean()), float(f.pow(2).mean().sqrt())])
        out["sdxl:sample:" + n] = f[::max(1, f.numel() // 2048)][:2048].numpy()
    path = os.path.join(REPO, "tests", "golden", "g19_vae_encoder_janus.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in ("ds:out", "enc:moments", "sdxl:moments"):
        v = out[k]
        print(f"  {k:14s} {v.shape} rms {float(np.sqrt((v.astype(np.float64) ** 2).mean())):.3f}")


if __name__ == "__main__":
    main()

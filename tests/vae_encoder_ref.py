"""Test-only fp32 restatement of diffusers' AutoencoderKL ENCODE path (diffusers 0.2x models/autoencoders/vae.py ``Encoder`` and the
``quant_conv`` of autoencoder_kl.py) in ``torch.nn.functional`` calls, on diffusers key names:

    conv_in 3x3 -> per level: layers_per_block ResnetBlock2D, then Downsample2D(padding=0) = F.pad(x, (0, 1, 0, 1)) + 3x3 stride-2 conv
    (every level but the last) -> mid block (resnet, single-head attention, resnet) -> GroupNorm(eps 1e-6) + SiLU -> conv_out 3x3
    -> quant_conv 1x1  =  the moments (mean | logvar)

The resnet / attention / GroupNorm pieces are oracle/vae_ref.py's (pinned against transformers' Janus blocks by g18); this file adds the
encoder wiring, itself pinned against transformers' ``JanusVQVAEEncoder`` by g19 (tools/gen_golden_vae_encoder.py).
"""
import torch
import torch.nn.functional as F

from oracle.vae_ref import TorchRefVaeDecoder


class TorchRefVaeEncoder(TorchRefVaeDecoder):
    def __init__(self, cfg, state_dict):
        c = cfg if isinstance(cfg, dict) else cfg.__dict__
        super().__init__({**c, "use_post_quant_conv": False}, state_dict)
        self.qc = c.get("use_quant_conv", True)

    def _downsample(self, x, p):
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), self.w[p + ".conv.weight"], self.w[p + ".conv.bias"], stride=2)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, keep_stages: bool = False) -> torch.Tensor:
        self.stages = []
        keep = (lambda n, t: self.stages.append((n, t.clone()))) if keep_stages else (lambda n, t: None)
        x = self._conv(x.to(torch.float32), "encoder.conv_in", 1)
        keep("conv_in", x)
        nb = len(self.boc)
        for i in range(nb):
            for j in range(self.layers):
                x = self._resnet(x, f"encoder.down_blocks.{i}.resnets.{j}")
                keep(f"down{i}.res{j}", x)
            if i != nb - 1:
                x = self._downsample(x, f"encoder.down_blocks.{i}.downsamplers.0")
                keep(f"down{i}.downsample", x)
        x = self._mid(x, "encoder.mid_block", keep)
        x = F.silu(self._gn(x, "encoder.conv_norm_out"))
        keep("norm_out", x)
        x = self._conv(x, "encoder.conv_out", 1)
        if self.qc:
            x = self._conv(x, "quant_conv", 0)
        return x

    __call__ = encode

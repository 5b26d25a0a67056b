"""CPU: the VAE-encoder surface (transformer_latent_diffusion_amd/vae_encoder.py) -- key spec, synthetic weights, the fp32 restatement
(tests/vae_encoder_ref.py) against transformers' published Janus encoder (fixture g19), DiagonalGaussianDistribution, state-dict routing
and the no-CPU-path failure."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_rms
from vae_encoder_ref import TorchRefVaeEncoder

from transformer_latent_diffusion_amd.vae import VaeDecoderConfig, synth_vae_state_dict, vae_decoder_spec
from transformer_latent_diffusion_amd.vae_encoder import (AutoencoderKL, AutoencoderKLEncoder, DiagonalGaussianDistribution,
                                                          VaeEncoderConfig, read_vae_encoder_config, synth_vae_encoder_state_dict,
                                                          vae_encoder_spec)

REF_TOL = 1e-5          # rel-rms: the fp32 restatement against the fp32 Janus modules (summation order only)


def _image(seed, shape, checksum):
    x = (torch.randn(*[int(s) for s in shape], generator=torch.Generator().manual_seed(int(seed))) * 0.6).clamp(-1.0, 1.0)
    f = x.double().reshape(-1)
    assert np.allclose([float(f.sum()), float(f.pow(2).sum()), float(f.abs().max())], checksum, rtol=1e-9, atol=1e-6)
    return x


def test_spec_keys_order_and_sdxl_parameter_count():
    spec = vae_encoder_spec(VaeEncoderConfig())
    keys = list(spec)
    assert keys[0] == "encoder.conv_in.weight" and keys[-2:] == ["quant_conv.weight", "quant_conv.bias"]
    assert spec["encoder.conv_in.weight"] == (128, 3, 3, 3) and spec["encoder.conv_out.weight"] == (8, 512, 3, 3)
    assert spec["encoder.down_blocks.1.resnets.0.conv_shortcut.weight"] == (256, 128, 1, 1)
    assert spec["encoder.down_blocks.2.downsamplers.0.conv.weight"] == (512, 512, 3, 3)
    assert "encoder.down_blocks.3.downsamplers.0.conv.weight" not in spec          # the last level keeps its resolution
    assert keys.index("encoder.mid_block.resnets.0.norm1.weight") < keys.index("encoder.mid_block.attentions.0.to_q.weight") \
        < keys.index("encoder.mid_block.resnets.1.norm1.weight") < keys.index("encoder.conv_norm_out.weight")
    n = {k: int(np.prod(s)) for k, s in spec.items()}
    assert sum(v for k, v in n.items() if k.startswith("encoder.")) == 34_163_592
    assert n["quant_conv.weight"] + n["quant_conv.bias"] == 72
    assert not any(k.startswith(("decoder.", "post_quant_conv.")) for k in spec)


def test_synthetic_weights_are_deterministic_and_leave_the_decoder_stream_alone():
    cfg = VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1)
    a, b, c = synth_vae_encoder_state_dict(cfg, 3), synth_vae_encoder_state_dict(cfg, 3), synth_vae_encoder_state_dict(cfg, 4)
    assert list(a) == list(vae_encoder_spec(cfg))
    assert all(np.array_equal(a[k], b[k]) and a[k].dtype == np.float32 for k in a)
    assert not np.array_equal(a["encoder.conv_in.weight"], c["encoder.conv_in.weight"])
    d = synth_vae_state_dict(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), 3)
    assert list(d) == list(vae_decoder_spec(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1)))


def test_restatement_matches_janus_downsampler():
    g = load_golden("g19_vae_encoder_janus.npz")
    sd = synth_vae_encoder_state_dict(VaeEncoderConfig(block_out_channels=tuple(g["tiny_boc"]), layers_per_block=int(g["tiny_layers"])),
                                      int(g["tiny_seed"]))
    ref = TorchRefVaeEncoder(VaeEncoderConfig(block_out_channels=tuple(g["tiny_boc"])), sd)
    got = ref._downsample(torch.from_numpy(g["ds:x"]), "encoder.down_blocks.0.downsamplers.0")
    assert got.shape == g["ds:out"].shape == (2, 64, 5, 7)
    assert rel_rms(got.numpy(), g["ds:out"]) < REF_TOL


def test_restatement_matches_janus_encoder_per_stage_and_moments():
    g = load_golden("g19_vae_encoder_janus.npz")
    cfg = VaeEncoderConfig(block_out_channels=tuple(int(c) for c in g["tiny_boc"]), layers_per_block=int(g["tiny_layers"]))
    ref = TorchRefVaeEncoder(cfg, synth_vae_encoder_state_dict(cfg, int(g["tiny_seed"])))
    x = _image(g["enc:x_seed"], g["enc:x_shape"], g["enc:x_checksum"])
    m = ref.encode(x, keep_stages=True)
    assert rel_rms(m.numpy(), g["enc:moments"]) < REF_TOL
    names = [n for n, _ in ref.stages]
    assert names == [str(n) for n in g["enc:stage_names"]]
    for n, t in ref.stages:
        f = t.reshape(-1)
        assert rel_rms(f[::max(1, f.numel() // 8192)][:8192].numpy(), g["enc:sample:" + n]) < REF_TOL, n
        assert np.allclose([float(f.mean()), float(f.pow(2).mean().sqrt())], g["enc:stat:" + n], rtol=1e-4, atol=1e-5), n
    # the SDXL geometry: moments in full, stages by statistics + strided samples
    cfg2 = VaeEncoderConfig()
    ref2 = TorchRefVaeEncoder(cfg2, synth_vae_encoder_state_dict(cfg2, int(g["sdxl:seed"])))
    m2 = ref2.encode(_image(g["sdxl:x_seed"], g["sdxl:x_shape"], g["sdxl:x_checksum"]), keep_stages=True)
    assert rel_rms(m2.numpy(), g["sdxl:moments"]) < REF_TOL
    assert [n for n, _ in ref2.stages] == [str(n) for n in g["sdxl:stage_names"]]
    for n, t in ref2.stages:
        f = t.reshape(-1)
        assert rel_rms(f[::max(1, f.numel() // 2048)][:2048].numpy(), g["sdxl:sample:" + n]) < REF_TOL, n
        assert np.allclose([float(f.mean()), float(f.pow(2).mean().sqrt())], g["sdxl:stat:" + n], rtol=1e-4, atol=1e-5), n


def test_diagonal_gaussian_formulas_clamp_and_generator():
    g = torch.Generator().manual_seed(5)
    mom = torch.randn(2, 8, 4, 4, generator=g) * 3
    mom[:, 4:, 0, 0] = 50.0
    mom[:, 4:, 0, 1] = -80.0
    d = DiagonalGaussianDistribution(mom)
    mean, logvar = mom[:, :4], mom[:, 4:].clamp(-30.0, 20.0)
    assert torch.equal(d.mean, mean) and torch.equal(d.logvar, logvar) and torch.equal(d.mode(), mean)
    assert float(d.logvar.max()) == 20.0 and float(d.logvar.min()) == -30.0
    assert torch.allclose(d.std, torch.exp(0.5 * logvar)) and torch.allclose(d.var, torch.exp(logvar))
    s1 = d.sample(torch.Generator().manual_seed(9))
    s2 = d.sample(torch.Generator().manual_seed(9))
    noise = torch.randn(mean.shape, generator=torch.Generator().manual_seed(9))
    assert torch.equal(s1, s2) and torch.equal(s1, mean + torch.exp(0.5 * logvar) * noise)
    assert torch.allclose(d.kl(), 0.5 * torch.sum(mean ** 2 + torch.exp(logvar) - 1.0 - logvar, dim=[1, 2, 3]))


def _full_sd(enc_cfg, dec_cfg, seed=1):
    sd = {k: torch.from_numpy(v) for k, v in synth_vae_encoder_state_dict(enc_cfg, seed).items()}
    sd.update({k: torch.from_numpy(v) for k, v in synth_vae_state_dict(dec_cfg, seed).items()})
    return sd


def test_encoder_load_state_dict_ignores_decoder_keys_and_checks_the_rest():
    cfg = VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1)
    sd = _full_sd(cfg, VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), seed=7)
    enc = AutoencoderKLEncoder(cfg).load_state_dict(sd)
    assert torch.equal(enc.state_dict()["encoder.conv_in.weight"], sd["encoder.conv_in.weight"])
    assert not any(k.startswith("decoder.") for k in enc.state_dict())
    missing = dict(sd)
    del missing["encoder.conv_out.bias"]
    with pytest.raises(RuntimeError, match="missing keys"):
        AutoencoderKLEncoder(cfg).load_state_dict(missing)
    bad = dict(sd)
    bad["encoder.conv_in.weight"] = torch.zeros(64, 3, 5, 5)
    with pytest.raises(RuntimeError, match="size mismatch"):
        AutoencoderKLEncoder(cfg).load_state_dict(bad)
    with pytest.raises(RuntimeError, match="unexpected key"):
        AutoencoderKLEncoder(cfg).load_state_dict({**sd, "encoder.extra.weight": torch.zeros(1)})
    # pre-0.19 attention names, 1x1-conv shaped
    old = {}
    for k, v in sd.items():
        for a, b in ((".to_q.", ".query."), (".to_k.", ".key."), (".to_v.", ".value."), (".to_out.0.", ".proj_attn.")):
            if ".attentions." in k and a in k:
                k = k.replace(a, b)
                v = v.reshape(*v.shape, 1, 1) if v.dim() == 2 else v
        old[k] = v
    enc2 = AutoencoderKLEncoder(cfg).load_state_dict(old)
    a = "encoder.mid_block.attentions.0"
    assert torch.equal(enc2.state_dict()[a + ".to_out.0.weight"], sd[a + ".to_out.0.weight"])


def test_autoencoder_kl_routes_keys_and_has_no_cpu_path():
    ecfg, dcfg = VaeEncoderConfig(), VaeDecoderConfig()
    sd = _full_sd(ecfg, dcfg, seed=2)
    vae = AutoencoderKL(ecfg, dcfg).load_state_dict(sd)
    out = vae.state_dict()
    assert set(out) == set(sd)
    assert torch.equal(vae.encoder.state_dict()["quant_conv.weight"], sd["quant_conv.weight"])
    assert torch.equal(vae.decoder.state_dict()["post_quant_conv.weight"], sd["post_quant_conv.weight"])
    assert sum(p.numel() for p in vae.parameters()) == sum(v.numel() for v in sd.values())
    with pytest.raises(RuntimeError, match="unexpected key"):
        AutoencoderKL(ecfg, dcfg).load_state_dict({**sd, "bogus.weight": torch.zeros(1)})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU path"):
            vae.encode(torch.zeros(1, 3, 64, 64))
        with pytest.raises(RuntimeError, match="no CPU path"):
            vae.decode(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        AutoencoderKLEncoder(VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1)).encode(torch.zeros(1, 3, 64, 64))


def test_config_reader(tmp_path):
    import json
    (tmp_path / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "in_channels": 3, "latent_channels": 4,
                                                      "block_out_channels": [128, 256, 512, 512], "layers_per_block": 2,
                                                      "norm_num_groups": 32, "use_quant_conv": True, "scaling_factor": 0.13025}))
    cfg = read_vae_encoder_config(str(tmp_path))
    assert cfg == VaeEncoderConfig()
    assert read_vae_encoder_config(str(tmp_path / "config.json")) == cfg

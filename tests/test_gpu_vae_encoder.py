"""GPU: the VAE-encode path (tld/data.py: images -> latents) through the C ABI (tld_vae_enc_* / tld_debug_conv3x3_s2) and the Python surface.

Pins: transformers' JanusVQVAEEncoder (fixture g19, tools/gen_golden_vae_encoder.py) and the fp32 restatement tests/vae_encoder_ref.py (itself
held to g19 at 1e-5 on the CPU).  Tolerances are the decoder's (tests/test_gpu_vae.py): the stride-2 convolution alone is the exact fp32
product of bf16 operands (CONV_TOL, accumulation order only); the encoder keeps bf16 activations between its layers (VAE_STAGE_TOL per
stage, VAE_IMAGE_TOL on the moments)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, rel_rms
from test_gpu_parity import _dev
from vae_encoder_ref import TorchRefVaeEncoder

pytestmark = pytest.mark.gpu

CONV_TOL = 2e-5
VAE_STAGE_TOL = 2e-2
VAE_IMAGE_TOL = 3e-2


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# (H, W = OUTPUT size.)  256-wide tiles -- and with them the half-tile ring K loop, for cin a multiple of 128 -- are taken when cout % 256 == 0 and
# ceil(B H W / 256) * cout / 256 >= 192 (launch_gemm); everything else runs the two-stage K loop on 128-wide tiles.
@pytest.mark.parametrize("B,H,W,cin,cout", [
    (2, 4, 4, 64, 64),             # one partial tile, two-stage loop
    (3, 6, 10, 64, 136),           # ragged: non-square, rows do not fill tiles, N not a multiple of the tile
    (1, 16, 16, 64, 128),          # exactly one 256-row tile
    (2, 16, 16, 512, 8),           # conv_out-like width: 8 output channels
    (4, 100, 124, 128, 256),       # ring loop (194 tiles of 256 x 256), ragged non-square image
    (2, 112, 112, 256, 512),       # ring loop (196 tiles), 36 K-steps
    (2, 112, 112, 512, 512),       # ring loop (196 tiles), 72 K-steps
    (5, 24, 24, 512, 512),         # two-stage loop on 128-wide tiles, 72 K-steps
])
def test_stride2_conv3x3_matches_padded_conv2d(B, H, W, cin, cout):
    from transformer_latent_diffusion_amd import _lib
    g = torch.Generator().manual_seed(B * 1000 + H + W + cin + cout)
    x = torch.randn(B, cin, 2 * H, 2 * W, generator=g).to(torch.bfloat16)
    w = (torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(9 * cin)).to(torch.bfloat16)
    ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), stride=2)              # [B, cout, H, W]
    assert ref.shape == (B, cout, H, W)
    d = _dev()
    x_nhwc = x.permute(0, 2, 3, 1).contiguous().to(d)
    w_pk = w.permute(0, 2, 3, 1).contiguous().to(d)
    out = torch.full((B * H * W, cout), float("nan"), device=d, dtype=torch.float32)
    _lib.check(_lib.lib().tld_debug_conv3x3_s2(x_nhwc.data_ptr(), w_pk.data_ptr(), out.data_ptr(), B, H, W, cin, cout, _stream()),
               "tld_debug_conv3x3_s2")
    torch.cuda.synchronize()
    got = out.cpu().view(B, H, W, cout).permute(0, 3, 1, 2)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"conv3x3_s2 B{B} {H}x{W} {cin}->{cout}: rel-max {err:.2e}")
    assert err < CONV_TOL, err


def _encoder(cfg, seed, max_batch=2):
    from transformer_latent_diffusion_amd.vae_encoder import AutoencoderKLEncoder, synth_vae_encoder_state_dict
    enc = AutoencoderKLEncoder(cfg, max_batch=max_batch)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in synth_vae_encoder_state_dict(cfg, seed).items()})
    return enc


def _image(seed, shape):
    return (torch.randn(*[int(s) for s in shape], generator=torch.Generator().manual_seed(int(seed))) * 0.6).clamp(-1.0, 1.0)


def test_tiny_encoder_stage_by_stage_against_janus():
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    g = load_golden("g19_vae_encoder_janus.npz")
    cfg = VaeEncoderConfig(block_out_channels=tuple(int(c) for c in g["tiny_boc"]), layers_per_block=int(g["tiny_layers"]))
    enc = _encoder(cfg, int(g["tiny_seed"]))
    x = _image(g["enc:x_seed"], g["enc:x_shape"])
    ref = TorchRefVaeEncoder(cfg, enc.state_dict())
    ref.encode(x, keep_stages=True)                  # (held to g19 at 1e-5 by tests/test_vae_encoder_host.py)
    full = dict(ref.stages)
    x = x.to(_dev())
    enc.moments(x)
    enc.set_debug(True)
    m = enc.moments(x)
    torch.cuda.synchronize()
    rep = []
    for n in (str(v) for v in g["enc:stage_names"]):
        t = enc.read_stage(n)
        f = t.reshape(-1)
        e = rel_rms(f[::max(1, f.numel() // 8192)][:8192].numpy(), g["enc:sample:" + n])       # the Janus stage, strided sample
        e_full = rel_rms(t.numpy(), full[n].numpy())                                                 # every value, via the restatement
        rep.append((n, e, e_full))
        assert e < VAE_STAGE_TOL and e_full < VAE_STAGE_TOL, (n, e, e_full)
    e = rel_rms(m.cpu().numpy(), g["enc:moments"])
    print("vae encoder vs janus (tiny; sample / full): " + ", ".join(f"{n} {a:.2e} / {b:.2e}" for n, a, b in rep) + f" | moments {e:.2e}")
    assert m.shape == (1, 8, 32, 32) and e < VAE_IMAGE_TOL, e


def test_sdxl_geometry_64px_against_janus():
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    g = load_golden("g19_vae_encoder_janus.npz")
    enc = _encoder(VaeEncoderConfig(), int(g["sdxl:seed"]), max_batch=1)
    x = _image(g["sdxl:x_seed"], g["sdxl:x_shape"]).to(_dev())
    enc.moments(x)
    enc.set_debug(True)
    m = enc.moments(x)
    torch.cuda.synchronize()
    rep = []
    for n in (str(v) for v in g["sdxl:stage_names"]):
        f = enc.read_stage(n).reshape(-1)
        e = rel_rms(f[::max(1, f.numel() // 2048)][:2048].numpy(), g["sdxl:sample:" + n])
        rep.append((n, e))
        assert e < VAE_STAGE_TOL * 1.25, (n, e)          # a 2048-element sample: its rel-rms scatters around the full tensor's
    e = rel_rms(m.cpu().numpy(), g["sdxl:moments"])
    print("vae encoder vs janus (SDXL geometry, 64 px): " + ", ".join(f"{n} {v:.2e}" for n, v in rep) + f" | moments {e:.2e}")
    assert m.shape == (1, 8, 8, 8) and e < VAE_IMAGE_TOL, e


@pytest.mark.parametrize("S,B", [(256, 2), (512, 1)])
def test_sdxl_geometry_against_the_restatement(S, B):
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    cfg = VaeEncoderConfig()
    enc = _encoder(cfg, 51 + S, max_batch=B)
    x = _image(60 + S, (B, 3, S, S))
    m = enc.moments(x.to(_dev())).cpu()
    want = TorchRefVaeEncoder(cfg, enc.state_dict()).encode(x)
    e = rel_rms(m.numpy(), want.numpy())
    print(f"vae encoder SDXL geometry {S} px x {B}: moments rel-rms {e:.2e}")
    assert m.shape == (B, 8, S // 8, S // 8) and torch.isfinite(m).all() and e < VAE_IMAGE_TOL, e


def _tiny_cfg():
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    return VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1)


def test_deterministic_and_batch_independent():
    cfg = _tiny_cfg()
    enc = _encoder(cfg, 8, max_batch=5)
    x = _image(70, (5, 3, 128, 128)).to(_dev())
    a, b = enc.moments(x), enc.moments(x)
    assert torch.equal(a, b)
    for k in range(5):
        assert torch.equal(enc.moments(x[k:k + 1].contiguous())[0], a[k]), k
    want = TorchRefVaeEncoder(cfg, enc.state_dict()).encode(x.cpu())
    assert rel_rms(a.cpu().numpy(), want.numpy()) < VAE_IMAGE_TOL


def test_input_dtypes():
    cfg = _tiny_cfg()
    enc = _encoder(cfg, 9, max_batch=2)
    ref = TorchRefVaeEncoder(cfg, enc.state_dict())
    x = _image(71, (2, 3, 64, 64))
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        xd = x.to(dt)
        m = enc.moments(xd.to(_dev())).cpu()
        e = rel_rms(m.numpy(), ref.encode(xd.float()).numpy())
        print(f"vae encoder input {dt}: moments rel-rms {e:.2e}")
        assert e < VAE_IMAGE_TOL, (dt, e)


def test_batches_above_the_engine_limit_are_chunked():
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig, encoder_batch_limit
    assert encoder_batch_limit(VaeEncoderConfig(), 1024) == 15          # one 128-channel 1024^2 bf16 activation: 256 MiB per image
    cfg = _tiny_cfg()
    enc = _encoder(cfg, 10, max_batch=2)
    x = _image(72, (5, 3, 64, 64)).to(_dev())
    m = enc.moments(x)
    assert enc._engine_key[2] == 2
    whole = _encoder(cfg, 10, max_batch=5).moments(x)
    assert torch.equal(m, whole)


def test_latent_dist_sample_and_mode():
    from transformer_latent_diffusion_amd.vae_encoder import DiagonalGaussianDistribution
    enc = _encoder(_tiny_cfg(), 11)
    x = _image(73, (2, 3, 64, 64)).to(_dev())
    out = enc.encode(x)
    dist = out.latent_dist
    assert isinstance(dist, DiagonalGaussianDistribution) and enc.encode(x, return_dict=False)[0].mean.shape == (2, 4, 32, 32)
    m = enc.moments(x)
    assert torch.equal(dist.mode(), m[:, :4])
    s = dist.sample(torch.Generator(device=_dev()).manual_seed(5))
    noise = torch.randn((2, 4, 32, 32), generator=torch.Generator(device=_dev()).manual_seed(5), device=_dev())
    assert s.device.type == "cuda" and torch.equal(s, m[:, :4] + torch.exp(0.5 * m[:, 4:].clamp(-30, 20)) * noise)


def test_error_paths():
    from transformer_latent_diffusion_amd import _lib
    enc = _encoder(_tiny_cfg(), 12)
    with pytest.raises(ValueError):
        enc.moments(torch.zeros(1, 4, 64, 64, device=_dev()))
    with pytest.raises(ValueError):
        enc.moments(torch.zeros(1, 3, 96, 96, device=_dev()))
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc.moments(torch.zeros(1, 3, 64, 64))
    L = _lib.lib()
    cc = _lib.TldVaeEncConfig()
    cc.in_channels, cc.latent_channels, cc.n_blocks = 3, 4, 2
    cc.block_out_channels[0], cc.block_out_channels[1] = 64, 128
    cc.layers_per_block, cc.norm_num_groups, cc.mid_block_attention, cc.use_quant_conv = 1, 32, 1, 1
    cc.image_size, cc.max_batch, cc.device_id = 96, 1, 0
    h = C.c_void_p()
    assert L.tld_vae_enc_create(C.byref(cc), C.byref(h)) != 0 and h.value is None
    assert b"image_size" in L.tld_last_error()
    cc.image_size, cc.max_batch = 1024, 64                          # 64 x 128 MiB x 2 per activation buffer: above 4 GiB
    assert L.tld_vae_enc_create(C.byref(cc), C.byref(h)) != 0 and b"4 GiB" in L.tld_last_error()


def test_images_to_latents_to_a_training_step():
    """tld/data.py encode_image on 128-px images -> 16 x 16 latents -> one Trainer.train_step: the images -> training path end to end."""
    from transformer_latent_diffusion_amd import AutoencoderKL, DenoiserConfig, Trainer, encode_image
    from transformer_latent_diffusion_amd.vae import VaeDecoderConfig
    from transformer_latent_diffusion_amd.vae_encoder import VaeEncoderConfig
    vae = AutoencoderKL(VaeEncoderConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1),
                        VaeDecoderConfig(block_out_channels=(64, 128, 128, 128), layers_per_block=1), init_seed=3, max_batch=4).to(_dev())
    img = torch.rand(4, 3, 128, 128, generator=torch.Generator().manual_seed(74)).to(_dev())
    with pytest.warns(RuntimeWarning):
        z = encode_image(img, vae, generator=torch.Generator(device=_dev()).manual_seed(1))
    assert z.shape == (4, 4, 16, 16) and torch.isfinite(z).all()
    tr = Trainer(DenoiserConfig(image_size=16, n_channels=4, n_layers=1), device=_dev(), init_seed=2, max_batch=4)
    y = torch.randn(4, 768, generator=torch.Generator().manual_seed(75))
    loss = tr.train_step((z / 8.0).cpu(), y)                           # (host batches, as the reference's loader yields them)
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()


def test_two_engines_in_one_process_have_independent_cores():
    """An AutoencoderKL's decoder and encoder engines alive together: interleaved calls, debug capture on the encoder only, and a rebuilt
    encoder engine leave each half bitwise equal to a stand-alone object with the same weights, and each engine's weight bytes alone."""
    from transformer_latent_diffusion_amd import AutoencoderKL
    from transformer_latent_diffusion_amd.vae import AutoencoderKLDecoder, VaeDecoderConfig
    from transformer_latent_diffusion_amd.vae_encoder import AutoencoderKLEncoder
    ecfg, dcfg = _tiny_cfg(), VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1)
    vae = AutoencoderKL(ecfg, dcfg, init_seed=5, max_batch=2).to(_dev())
    x = _image(76, (2, 3, 64, 64)).to(_dev())
    z = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77)).to(_dev())
    with pytest.warns(RuntimeWarning):
        want_img = AutoencoderKLDecoder(dcfg, init_seed=5, max_batch=2).decode(z)[0]
        want_mom = AutoencoderKLEncoder(ecfg, init_seed=5, max_batch=2).moments(x)
        img0 = vae.decode(z)[0]
        dec_bytes = vae.decoder.weight_bytes
        vae.encoder._ensure_engine(x.device, 64)
        vae.encoder.set_debug(True)
        mom0 = vae.encoder.moments(x)
    enc_bytes = vae.encoder.weight_bytes
    img1 = vae.decode(z)[0]
    assert dec_bytes > 0 and enc_bytes > 0 and vae.decoder.weight_bytes == dec_bytes and vae.encoder.weight_bytes == enc_bytes
    assert vae.encoder.read_stage("mid.attn").shape == (2, 128, 32, 32)
    for name in ("conv_in", "mid.res0", "mid.attn", "mid.res1", "up0.res0", "norm_out", "down0.res0"):
        with pytest.raises(RuntimeError, match="no captured stage named"):
            vae.decoder.read_stage(name)
    vae.encoder._drop_engine()
    assert vae.encoder._engine is None and vae.decoder._engine is not None
    mom1 = vae.encoder.moments(x)
    torch.cuda.synchronize()
    assert vae.encoder.weight_bytes == enc_bytes and vae.decoder.weight_bytes == dec_bytes
    assert torch.equal(img0, want_img) and torch.equal(img1, want_img)
    assert torch.equal(mom0, want_mom) and torch.equal(mom1, want_mom)


def test_conv_hooks_refuse_oversized_operands_with_a_status():
    """Both debug convolution hooks run one body: a source image of 4 GiB or more is refused before anything is allocated or launched, with
    a non-zero status, tld_last_error set and the output untouched.  (No argument of either hook reaches a refusal by launch_gemm itself:
    its operand-reach check covers plain GEMMs only, EPI_F32 convolutions exist at both tile widths, and a hook sets cv_up or cv_down, never
    both; the body passes that status on all the same.)"""
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    d = _dev()
    x = torch.zeros(64, dtype=torch.bfloat16, device=d)
    w = torch.zeros(8 * 9 * 64, dtype=torch.bfloat16, device=d)
    out = torch.full((8,), float("nan"), device=d)
    for call in (lambda: L.tld_debug_conv3x3(x.data_ptr(), w.data_ptr(), out.data_ptr(), 8, 4096, 4096, 64, 8, 0, _stream()),     # 16 GiB of source
                 lambda: L.tld_debug_conv3x3_s2(x.data_ptr(), w.data_ptr(), out.data_ptr(), 8, 2048, 2048, 64, 8, _stream())):
        rc = call()
        assert rc != 0 and b"4 GiB" in L.tld_last_error(), (rc, L.tld_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(out).all()

"""GPU tests of the BASELINE configurations at their real sizes and of the pipeline / multi-rank shells.

C1: 100 M model, 32x32x4 latents, 35 steps + CFG 6, 64 images (model batch 128) -- the bench workload itself.
C2: the same sampler sharded over ranks (two ranks on ONE GPU here, gloo plumbing; RCCL is exercised by the
    driver's multi-GPU run) with tld_sample as the per-rank sampler.
C3: image_size 64 (1024 tokens), 16 images.
Plus: the reference's seed= path, the text-to-image shell, and the LayerNorm stress fixture.
Tolerances as in test_gpu_parity.py (forward 2e-2, trajectory 6e-2 rel-rms vs the fp32 reference).
"""
import json
import os
import subprocess
import sys
from dataclasses import asdict

import numpy as np
import pytest
import torch

from conftest import cfg_from_arr, load_golden, rel_rms, synth_weights
from test_gpu_parity import CFG_FWD_REG, FWD_REG, FWD_TOL, TRAJ_REG, TRAJ_TOL, _dev, _engine, _t, held, held_key

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(TESTS)


def test_seed_path_reproduces_reference_latent():
    """generate(seed=10) draws x_T exactly as the reference's CPU path does (bit-exact, see test_host_logic) and
    lands on the reference's end latent within the trajectory tolerance (g2 ``seed10_latent``)."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    g = load_golden("g2_tiny32_sampler.npz")
    cfg, sd, m = _engine(g)
    gen = DiffusionGenerator(m, None, _dev(), torch.float32)
    x_T = gen.initialize_image(None, 2, 32, 10)
    assert x_T.device.type == "cuda" and np.array_equal(x_T.cpu().numpy(), g["seed10_xT"])
    lat = gen.generate_latents(torch.from_numpy(g["labels"]), n_iter=5, num_imgs=2, class_guidance=3.0, seed=10,
                               img_size=32, sharp_f=0.0, bright_f=0.0)
    held_key(rel_rms(lat.cpu().numpy(), g["seed10_latent"]), TRAJ_TOL, "g2/seed10_end_latent", TRAJ_REG)


def test_text_to_image_shell():
    """DiffusionTransformer.generate_image_from_text with injected text encoder / VAE stand-ins returns a PIL image
    of the grid's size (mirrors the reference's test_full_generation_pipeline, tests/test_diffuser.py:88-93)."""
    from PIL import Image
    from transformer_latent_diffusion_amd import DenoiserConfig, DiffusionTransformer, LTDConfig

    class FakeVAE:                                   # 8x upsampling decoder stand-in: latent [B,4,S,S] -> image [B,3,8S,8S]
        def decode(self, z):
            return (torch.tanh(z[:, :3]).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3),)

    calls = []

    def text_encoder(prompts):                       # pooled-CLIP stand-in: one 768-vector per prompt
        calls.append(list(prompts))
        g = torch.Generator().manual_seed(len(prompts[0]))
        return torch.randn(len(prompts), 768, generator=g) * 0.5

    cfg = LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4))          # default tiny model, 16x16 latents
    pipe = DiffusionTransformer(cfg, vae=FakeVAE(), text_encoder=text_encoder, run_device=_dev())
    out = pipe.generate_image_from_text(prompt="a cute cat", seed=11, n_iter=5)
    assert isinstance(out, Image.Image) and out.size == (128, 128) and out.mode == "RGB"
    assert calls[-1] == ["a cute cat"]
    out4 = pipe.generate_image_from_text(prompt="a cute cat", num_imgs=4, seed=11, n_iter=5, img_size=999)   # img_size ignored (:175)
    assert out4.size == (2 * 132 + 4, 2 * 132 + 4)
    # same seed, same prompt -> same picture; the first tile of the grid is the single image (same noise row 0)
    again = pipe.generate_image_from_text(prompt="a cute cat", seed=11, n_iter=5)
    assert np.array_equal(np.asarray(out), np.asarray(again))
    assert np.array_equal(np.asarray(out4)[4:132, 4:132], np.asarray(out))


def test_batched_text_to_image_front_edge():
    """generate_images_from_texts / RequestBatcher: several prompts, one sampler call; each picture equals the
    single-prompt call with the same prompt and seed (pixel-exact: samples never interact)."""
    from PIL import Image
    from transformer_latent_diffusion_amd import DenoiserConfig, DiffusionTransformer, LTDConfig, RequestBatcher

    class FakeVAE:
        def decode(self, z):
            return (torch.tanh(z[:, :3]).repeat_interleave(8, dim=2).repeat_interleave(8, dim=3),)

    def text_encoder(prompts):                       # deterministic per prompt, independent of the batch it arrives in
        rows = [torch.randn(768, generator=torch.Generator().manual_seed(sum(map(ord, p)))) * 0.5 for p in prompts]
        return torch.stack(rows).to(_dev())          # stays on the device

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=FakeVAE(), text_encoder=text_encoder,
                                run_device=_dev())
    prompts, seeds = ["a cute cat", "a red car", "tree"], [11, 5, 7]
    imgs = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5)
    assert len(imgs) == 3 and all(isinstance(im, Image.Image) and im.size == (128, 128) for im in imgs)
    for p, s, im in zip(prompts, seeds, imgs):
        single = pipe.generate_image_from_text(prompt=p, seed=s, n_iter=5)
        assert np.array_equal(np.asarray(single), np.asarray(im)), p
    rb = RequestBatcher(pipe, max_batch=8)
    tickets = [rb.submit(p, 6, s, 5) for p, s in zip(prompts, seeds)] + [rb.submit("tree", 3, 7, 5)]
    out = rb.flush()
    assert all(np.array_equal(np.asarray(out[t]), np.asarray(im)) for t, im in zip(tickets[:3], imgs))
    assert not np.array_equal(np.asarray(out[tickets[3]]), np.asarray(imgs[2]))            # other guidance, other picture
    assert pipe.generate_images_from_texts([]) == []


def test_c1_full_size_sampler_vs_reference_trajectory():
    """The bench workload itself (64 images, 35 steps, CFG 6: share-L0 fan-out, 384-wide down tiles, XCD grid -- all
    only active at this size): sample 0 carries the g5 trajectory inputs and must land on the reference's end latent,
    with the same bits as the batch-1 run."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    g = load_golden("g5_100m.npz")
    cfg, sd, m = _engine(g)
    gen = DiffusionGenerator(m, None, _dev(), torch.float32)
    B = 64
    rng = torch.Generator().manual_seed(64)
    seeds = torch.randn(B, 4, 32, 32, generator=rng)
    labels = torch.randn(B, 768, generator=rng) * 0.5
    seeds[0], labels[0] = torch.from_numpy(g["traj_seeds"][0]), torch.from_numpy(g["traj_labels"][0])
    kw = dict(n_iter=int(g["traj_n_iter"]), class_guidance=float(g["traj_class_guidance"]), img_size=32, sharp_f=0.0, bright_f=0.0)
    full = gen.generate_latents(labels, num_imgs=B, seeds=seeds, **kw)
    assert torch.isfinite(full).all()
    held(rel_rms(full[:1].cpu().numpy(), g["traj_latent"]), TRAJ_TOL, TRAJ_REG, "C1 end latent of the golden sample inside the 64-image batch")
    one = gen.generate_latents(labels[:1], num_imgs=1, seeds=seeds[:1], **kw)
    assert torch.equal(one[0], full[0])
    assert torch.equal(full, gen.generate_latents(labels, num_imgs=B, seeds=seeds, **kw))      # deterministic


def test_c3_sampler_512px():
    """BASELINE C3: image_size 64 (1024 tokens), 16 images, 35 steps + CFG 6 vs the reference trajectory (g11)."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    g = load_golden("g11_100m_512px_traj.npz")
    cfg, sd, m = _engine(g)
    gen = DiffusionGenerator(m, None, _dev(), torch.float32)
    B = 16
    rng = torch.Generator().manual_seed(16)
    seeds = torch.randn(B, 4, 64, 64, generator=rng)
    labels = torch.randn(B, 768, generator=rng) * 0.5
    seeds[0], labels[0] = torch.from_numpy(g["traj_seeds"][0]), torch.from_numpy(g["traj_labels"][0])
    kw = dict(n_iter=int(g["traj_n_iter"]), class_guidance=float(g["traj_class_guidance"]), img_size=64, sharp_f=0.0, bright_f=0.0)
    one, tx0, _ = gen.generate_latents(labels[:1], num_imgs=1, seeds=seeds[:1], trace=True, **kw)
    held(rel_rms(tx0[0].cpu().numpy(), g["traj_x0_first"]), FWD_TOL, CFG_FWD_REG, "C3 first CFG prediction")
    held(rel_rms(one.cpu().numpy(), g["traj_latent"]), TRAJ_TOL, TRAJ_REG, "C3 35-step end latent")
    full = gen.generate_latents(labels, num_imgs=B, seeds=seeds, **kw)
    assert torch.isfinite(full).all() and torch.equal(full[0], one[0])


def test_c4_sampler_1024px_bf16():
    """BASELINE C4 shape in bf16: image_size 128 (4096 tokens), 35 steps + CFG 6 vs the reference's fp32 trajectory (g14); the
    MX-fp8 GEMM mode is held against the same fixture in test_gpu_fp8.py."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    g = load_golden("g14_100m_1024px_traj.npz")
    cfg, sd, m = _engine(g)
    gen = DiffusionGenerator(m, None, _dev(), torch.float32)
    kw = dict(n_iter=int(g["traj_n_iter"]), class_guidance=float(g["traj_class_guidance"]), img_size=128, sharp_f=0.0, bright_f=0.0)
    one, tx0, _ = gen.generate_latents(torch.from_numpy(g["traj_labels"]), num_imgs=1, seeds=torch.from_numpy(g["traj_seeds"]), trace=True, **kw)
    e0 = rel_rms(tx0[0].cpu().numpy(), g["traj_x0_first"])
    r = rel_rms(one.cpu().numpy(), g["traj_latent"])
    print(f"C4 bf16: first CFG prediction rel-rms {e0:.2e}, 35-step end latent {r:.2e}")
    held(e0, FWD_TOL, CFG_FWD_REG, "C4 bf16 first CFG prediction")
    held(r, TRAJ_TOL, TRAJ_REG, "C4 bf16 35-step end latent")


@pytest.mark.parametrize("image_size,d", [(24, 256), (40, 128)])
def test_sampler_on_grids_without_a_specialised_attention_kernel(image_size, d):
    """A 6-step CFG DPM-Solver++(2M) sample on 12 x 12 / 20 x 20 token grids (masked chunked attention, tiled depthwise kernel, no fused paths) against the
    C restatement's sampler on the same noise and labels: the trajectory tolerance of the golden runs."""
    from oracle.oracle import OracleDenoiser
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator, schedule
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = DenoiserConfig(image_size=image_size, n_channels=4, embed_dim=d, n_layers=2)
    sd = synth_state_dict(cfg, 71)
    dev = _dev()
    model = Denoiser(**asdict(cfg)).to(dev)
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    g = torch.Generator().manual_seed(72)
    x = torch.randn(3, 4, image_size, image_size, generator=g)
    label = torch.randn(3, 768, generator=g) * 0.5
    gen = DiffusionGenerator(model, None, dev, torch.float32)
    lat = gen.generate_latents(label, n_iter=6, num_imgs=3, class_guidance=4.0, seeds=x, sharp_f=0.0, bright_f=0.0, img_size=image_size)
    ref = OracleDenoiser(cfg, sd).sample(x.numpy(), label.numpy(), schedule.noise_schedule(6, 1), 4.0, True, 0.0, 0.0)
    r = rel_rms(lat.cpu().numpy(), ref)
    print(f"{image_size // 2} x {image_size // 2} tokens, d = {d}: 6-step CFG end latent rel-rms {r:.2e}")
    assert np.isfinite(lat.cpu().numpy()).all()
    held_key(r, TRAJ_TOL, f"oracle_sampler/{image_size}px_d{d}", TRAJ_REG)


def test_checkpoint_file_into_engine_512px(tmp_path):
    """SURVEY 8(f2) on the device: a reference-format .pth of a 16x16-token (256 px) 100 M-width model is loaded into a 512 px model
    with load_checkpoint_into (README.md:23 workflow; tld/diffusion.py:148-155), the engine is built from it, and its forward
    equals, bit for bit, the forward of a model that was given the pre-resampled state_dict directly."""
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig
    from transformer_latent_diffusion_amd.checkpoint import load_checkpoint_into, upsample_pos_embed
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    small = DenoiserConfig(image_size=32, noise_embed_dims=256, patch_size=2, embed_dim=768, dropout=0, n_layers=2, text_emb_size=768,
                           n_channels=4, mlp_multiplier=4)
    big = DenoiserConfig(**{**asdict(small), "image_size": 64})
    sd = {k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(small, 21).items()}
    path = str(tmp_path / "state_dict_256px.pth")
    torch.save({"model_ema": {"_orig_mod." + k: v for k, v in sd.items()}, "opt_state": {}, "global_step": 7}, path)     # train.py:150-156 format
    a = Denoiser(**asdict(big))
    load_checkpoint_into(a, path)
    b = Denoiser(**asdict(big))
    b.load_state_dict(upsample_pos_embed(sd, 64))
    rng = torch.Generator().manual_seed(2)
    x = torch.randn(2, 4, 64, 64, generator=rng); sg = torch.rand(2, 1, generator=rng) * 0.9 + 0.05; lab = torch.randn(2, 768, generator=rng) * 0.5
    ya = a.to(_dev())(_t(x.numpy()), _t(sg.numpy()), _t(lab.numpy()))
    yb = b.to(_dev())(_t(x.numpy()), _t(sg.numpy()), _t(lab.numpy()))
    assert ya.shape == (2, 4, 64, 64) and torch.isfinite(ya).all() and torch.equal(ya, yb)
    # ... and both are the forward of the fp32 restatement on the resampled state_dict (a resampler / key-mapping slip common to the two
    # engine-side loads would cancel in the comparison above)
    from oracle.torch_ref import TorchRefDenoiser
    ref = TorchRefDenoiser(asdict(big), {k: v.numpy() for k, v in upsample_pos_embed(sd, 64).items()})(x, sg, lab).numpy()
    held_key(rel_rms(ya.cpu().numpy(), ref), FWD_TOL, "checkpoint_512px_vs_torch_ref", FWD_REG)
    # the table really was resampled (1024 rows from 256) and it matters: the un-resampled small model at its own size differs
    assert a.state_dict()["denoiser_trans_block.pos_embed.weight"].shape == (1024, 768)


def test_fused_qkv_attention_kernel_vs_golden_and_two_kernel_path(tmp_path):
    """EPI_QKV_ATTN (round 4): at 256 tokens the QKV projection and the whole self-attention of a (sample, head) are one GEMM tile + epilogue
    (tld/transformer_blocks.py:51-59 + 24-48); q | k / v^T never reach HBM.  Held against g5 (100 M forward, 35-step trajectory) with the
    kernel on and off (TLD_FUSE_QKV_ATTN, read when the engine is created -- a process each).  Both paths round q, k, v to bf16 from the same
    accumulators and run the same attention arithmetic: block 0's x + attention may differ in isolated bf16 ulps (contraction choices of two
    kernels), nothing more; and the fused forward is bit-reproducible and independent of the batch it travels in."""
    script = tmp_path / "fused.py"
    script.write_text(f"""
import sys, numpy as np, torch
sys.path.insert(0, {REPO!r}); sys.path.insert(0, {TESTS!r})
from dataclasses import asdict
from conftest import cfg_from_arr, load_golden, rel_rms, synth_weights
from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
g = load_golden("g5_100m.npz")
cfg = cfg_from_arr(g["cfg"]); sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
dev = torch.device("cuda:0")
m = Denoiser(**asdict(cfg)).to(dev); m.load_state_dict({{k: torch.from_numpy(np.array(v)) for k, v in sd.items()}})
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
out = m(t(g["x"]), t(g["sigma"]), t(g["label"])).cpu().numpy()
gen = DiffusionGenerator(m, None, dev, torch.float32)
lat = gen.generate_latents(torch.from_numpy(g["traj_labels"]), n_iter=35, num_imgs=1, class_guidance=6.0, seeds=torch.from_numpy(g["traj_seeds"]),
                           img_size=32, sharp_f=0.0, bright_f=0.0).cpu().numpy()
rng = np.random.default_rng(3)
x = rng.standard_normal((70, 4, 32, 32)).astype(np.float32); s = rng.uniform(0.02, 0.98, (70, 1)).astype(np.float32)
lab = (rng.standard_normal((70, 768)) * 0.5).astype(np.float32)
big = m(t(x), t(s), t(lab)).cpu().numpy()
again = m(t(x), t(s), t(lab)).cpu().numpy()
few = m(t(x[:3]), t(s[:3]), t(lab[:3])).cpu().numpy()
m.set_debug(True)
m(t(x[:4]), t(s[:4]), t(lab[:4]))
np.save(sys.argv[1], m.read_stage("blk0_sa", (4, 256, 768)))
print("RESULT", rel_rms(out, g["x0"]), rel_rms(lat, g["traj_latent"]), int(np.array_equal(big, again)), int(np.array_equal(big[:3], few)))
""")
    outs, sa = {}, {}
    for flag in ("1", "0"):
        dump = str(tmp_path / f"sa{flag}.npy")
        r = subprocess.run([sys.executable, str(script), dump], capture_output=True, text=True, env=dict(os.environ, TLD_FUSE_QKV_ATTN=flag), timeout=600)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        fwd, traj, rep, bind = r.stdout.split("RESULT")[1].split()[:4]
        outs[flag] = (float(fwd), float(traj))
        held(float(fwd), FWD_TOL, FWD_REG, f"g5 forward, TLD_FUSE_QKV_ATTN={flag}")
        held(float(traj), TRAJ_TOL, TRAJ_REG, f"g5 trajectory, TLD_FUSE_QKV_ATTN={flag}")
        assert int(rep) == 1 and int(bind) == 1, (flag, rep, bind)
        sa[flag] = np.load(dump)
    print("fused / two-kernel (forward, trajectory):", outs)
    diff = sa["1"] != sa["0"]
    assert diff.mean() <= 1e-4, diff.mean()                                            # isolated elements only ...
    assert np.abs(sa["1"] - sa["0"]).max() <= 2.0 ** -6 * np.abs(sa["0"]).max()        # ... by a bf16 ulp or two of the stored att


@pytest.mark.parametrize("M,N,K,ks", [(512, 768, 3072, 4), (300, 768, 3072, 4), (2048, 384, 1536, 4), (256, 768, 3072, 2), (1000, 200, 512, 8)])
def test_split_k_gemm_slices_sum_to_the_product(M, N, K, ks):
    """GemmParams::ksplit (round 5, the low-latency down projection): slice s is the exact fp32-accumulated product over K range s; the slices summed in
    fp64 equal the fp64 product of the bf16 operands to fp32 rounding; repeated runs give the same bits."""
    import ctypes as C
    from transformer_latent_diffusion_amd import _lib
    g = torch.Generator().manual_seed(M + N + K + ks)
    a = torch.randn(M, K, generator=g).to(torch.bfloat16).to(_dev())
    w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).to(_dev())
    c = torch.full((ks, M, N), float("nan"), device=_dev(), dtype=torch.float32)
    call = lambda out: _lib.check(_lib.lib().tld_debug_gemm_splitk(a.data_ptr(), w.data_ptr(), out.data_ptr(), M, N, K, ks,
                                                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "splitk")
    call(c)
    c2 = torch.empty_like(c); call(c2)
    torch.cuda.synchronize()
    assert torch.isfinite(c).all() and torch.equal(c, c2)
    kk = K // ks
    for s in range(ks):
        ref = a[:, s * kk:(s + 1) * kk].double() @ w[:, s * kk:(s + 1) * kk].double().t()
        err = (c[s].double() - ref).abs().max().item()
        assert err <= 2e-5 * ref.abs().max().item() * np.sqrt(kk / 64) + 1e-5, (s, err)
    full = a.double() @ w.double().t()
    assert (c.double().sum(0) - full).abs().max().item() <= 4e-5 * full.abs().max().item() * np.sqrt(K / 64) + 1e-5


@pytest.mark.parametrize("M,N,K,ks", [(512, 768, 3072, 8), (1024, 768, 3072, 4), (512, 384, 1536, 4)])
def test_split_k_small_launch_kernel_bitwise_equals_8_wave_kernel(M, N, K, ks, tmp_path):
    """Round 6: split-K launches with at most one 256 x 128 item per CU run on the 4-wave kernel of tld_updw.hip.  Its slices must be BITWISE those of the 8-wave
    two-stage kernel (same K order per output element) -- the low-latency classes' numerics do not depend on which kernel a batch size selects.  TLD_SPLITK_SMALL
    is read once per process: the 8-wave run is a subprocess."""
    import ctypes as C
    from transformer_latent_diffusion_amd import _lib
    code = ("import sys, ctypes as C, numpy as np, torch\n"
            "from transformer_latent_diffusion_amd import _lib\n"
            f"M, N, K, ks = {M}, {N}, {K}, {ks}\n"
            "g = torch.Generator().manual_seed(M + N + K + ks)\n"
            "a = torch.randn(M, K, generator=g).to(torch.bfloat16).cuda()\n"
            "w = (torch.randn(N, K, generator=g) * 0.1).to(torch.bfloat16).cuda()\n"
            "c = torch.full((ks, M, N), float('nan'), device='cuda', dtype=torch.float32)\n"
            "_lib.check(_lib.lib().tld_debug_gemm_splitk(a.data_ptr(), w.data_ptr(), c.data_ptr(), M, N, K, ks, C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'splitk')\n"
            "torch.cuda.synchronize(); np.save(sys.argv[1], c.cpu().numpy())\n")
    outs = {}
    for tag, env in (("small", {}), ("wave8", {"TLD_SPLITK_SMALL": "0"})):
        path = tmp_path / f"{tag}.npy"
        r = subprocess.run([sys.executable, "-c", code, str(path)], env=dict(os.environ, **env), capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = np.load(path)
    assert np.isfinite(outs["small"]).all() and np.array_equal(outs["small"], outs["wave8"])


@pytest.mark.parametrize("batch", [2, 6, 32])
def test_default_class_small_launch_down_projection_bitwise_equals_8_wave_kernel(batch, tmp_path):
    """Round 6: the default class's down projection (x += hid Wdown^T + b and the LayerNorm-1 partial sums, tld/transformer_blocks.py:104,138) of launches with at most one
    128 x 192 tile per CU runs on the 4-wave kernel of tld_updw.hip.  The forward output must be BITWISE that of the 8-wave 192- / 384-wide kernels -- the default class's
    results do not depend on which kernel a batch size selects.  TLD_DOWN_SMALL is read once per process: the 8-wave run is a subprocess."""
    code = ("import sys, numpy as np, torch\n"
            "sys.path.insert(0, 'tests')\n"
            "from dataclasses import asdict\n"
            "from conftest import cfg_from_arr, load_golden, synth_weights\n"
            "from transformer_latent_diffusion_amd import Denoiser\n"
            "g = load_golden('g5_100m.npz'); cfg = cfg_from_arr(g['cfg'])\n"
            "sd = synth_weights(cfg, g['weight_seed'], g['weight_checksum'])\n"
            "m = Denoiser(**asdict(cfg)).to(torch.device('cuda', 0)); m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})\n"
            f"B = {batch}; rng = np.random.default_rng(5); reps = -(-B // g['x'].shape[0])\n"
            "x = np.concatenate([g['x']] * reps)[:B] * rng.uniform(0.7, 1.3, (B, 1, 1, 1)).astype(np.float32)\n"
            "s = rng.uniform(0.05, 0.95, (B, 1)).astype(np.float32); lab = np.concatenate([g['label']] * reps)[:B]\n"
            "t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()\n"
            "np.save(sys.argv[1], m(t(x), t(s), t(lab)).float().cpu().numpy())\n")
    outs = {}
    for tag, env in (("small", {}), ("wave8", {"TLD_DOWN_SMALL": "0"})):
        path = tmp_path / f"{tag}.npy"
        r = subprocess.run([sys.executable, "-c", code, str(path)], env=dict(os.environ, **env), capture_output=True, text=True,
                           cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[tag] = np.load(path)
    assert np.isfinite(outs["small"]).all() and np.abs(outs["small"]).max() > 0 and np.array_equal(outs["small"], outs["wave8"])


def test_low_latency_class_vs_golden_and_inside_the_class():
    """Denoiser.set_low_latency (round 5; the reference serves one prompt per call, tld/app.py:48-65): split-K down projection for engines of at most
    4096 token rows.  Held against g5 exactly as the default class (forward, 35-step trajectory); bit-identical across batch sizes INSIDE the class;
    the two classes differ by fp32 summation order only; batches beyond the class capacity raise."""
    from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
    g = load_golden("g5_100m.npz")
    cfg = cfg_from_arr(g["cfg"]); sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
    sd_t = {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}
    ll = Denoiser(**asdict(cfg)).to(_dev()); ll.load_state_dict(sd_t); ll.set_low_latency(True)
    base = Denoiser(**asdict(cfg)).to(_dev()); base.load_state_dict(sd_t)
    out = ll(_t(g["x"]), _t(g["sigma"]), _t(g["label"])).cpu().numpy()
    held(rel_rms(out, g["x0"]), FWD_TOL, FWD_REG, "g5 forward, low-latency class")
    # the two classes differ in the fp32 summation order of ONE product per block: after block 0 that is isolated bf16 ulps of the residual stream; the
    # network then amplifies any perturbation to the level of its own bf16 rounding noise (the same happens between the fused and the two-kernel
    # attention paths), so at the output the classes are two realisations of that noise -- each held against the reference above / below
    ref = base(_t(g["x"]), _t(g["sigma"]), _t(g["label"])).cpu().numpy()
    ll.set_debug(True); base.set_debug(True)
    ll(_t(g["x"]), _t(g["sigma"]), _t(g["label"])); base(_t(g["x"]), _t(g["sigma"]), _t(g["label"]))
    b_ll, b_base = ll.read_stage("blk0_mlp", (2, 256, 768)), base.read_stage("blk0_mlp", (2, 256, 768))
    ll.set_debug(False); base.set_debug(False)
    flips = (b_ll != b_base).mean()
    assert flips <= 2e-2 and np.abs(b_ll - b_base).max() <= 2.0 ** -6 * np.abs(b_base).max(), (flips, np.abs(b_ll - b_base).max())
    assert not np.array_equal(out, ref) and rel_rms(out, ref) <= FWD_REG, rel_rms(out, ref)
    print(f"low-latency vs default class: block-0 residual differs in {flips:.2e} of its elements; forward outputs differ by {rel_rms(out, ref):.2e} rel-rms")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((14, 4, 32, 32)).astype(np.float32); s = rng.uniform(0.02, 0.98, (14, 1)).astype(np.float32)
    lab = (rng.standard_normal((14, 768)) * 0.5).astype(np.float32)
    big = ll(_t(x), _t(s), _t(lab)).cpu().numpy()                 # 14 x 256 = 3584 rows: the engine is rebuilt at that capacity, still inside the class
    few = ll(_t(x[:3]), _t(s[:3]), _t(lab[:3])).cpu().numpy()
    assert np.array_equal(big[:3], few) and np.array_equal(big, ll(_t(x), _t(s), _t(lab)).cpu().numpy())
    gen = DiffusionGenerator(ll, None, _dev(), torch.float32)
    lat = gen.generate_latents(torch.from_numpy(g["traj_labels"]), n_iter=35, num_imgs=1, class_guidance=6.0, seeds=torch.from_numpy(g["traj_seeds"]),
                               img_size=32, sharp_f=0.0, bright_f=0.0).cpu().numpy()
    held(rel_rms(lat, g["traj_latent"]), TRAJ_TOL, TRAJ_REG, "g5 trajectory, low-latency class")
    with pytest.raises(RuntimeError, match="low-latency class"):
        ll(_t(np.tile(x, (2, 1, 1, 1))[:20]), _t(np.tile(s, (2, 1))[:20]), _t(np.tile(lab, (2, 1))[:20]))      # 20 x 256 rows > 4096
    # the class is bf16-only -- an MX-fp8 engine refuses it (it used to accept and silently run the default down projection)
    f8 = Denoiser(**asdict(cfg)).to(_dev()).set_gemm_dtype("fp8").set_low_latency(True)
    f8.load_state_dict(sd_t)
    with pytest.raises(RuntimeError, match="low-latency class"):
        f8(_t(x[:1]), _t(s[:1]), _t(lab[:1]))
    # widths the finishing kernel does not take refuse the class instead of silently running the default one
    from transformer_latent_diffusion_amd import DenoiserConfig
    odd = Denoiser(**asdict(DenoiserConfig(image_size=32, n_channels=4, embed_dim=256, n_layers=1))).to(_dev()).set_low_latency(True)
    with pytest.raises(RuntimeError, match="low-latency class"):
        odd(torch.zeros(1, 4, 32, 32, device=_dev()), torch.full((1, 1), 0.5, device=_dev()), torch.zeros(1, 768, device=_dev()))


def test_low_latency_class_2_eight_splits():
    """Class 2 of Denoiser.set_low_latency (round 6): eight K-splits for engines of at most 1024 token rows -- the one-prompt-per-call pattern (tld/app.py:48-65).  Held against
    the reference's own forward like class 1, bit-identical across the batch sizes it admits, and refused beyond its capacity."""
    from transformer_latent_diffusion_amd import Denoiser
    g = load_golden("g5_100m.npz")
    cfg = cfg_from_arr(g["cfg"])
    sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
    m = Denoiser(**asdict(cfg)).to(_dev()).set_low_latency(2)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    x, s, lab = g["x"][:2], g["sigma"][:2], g["label"][:2]
    m.reserve(4)                                               # 4 x 256 = 1024 token rows: the class's capacity
    one = m(_t(x[:1]), _t(s[:1]), _t(lab[:1])).cpu().numpy()
    out = m(_t(x), _t(s), _t(lab)).cpu().numpy()
    four = m(_t(np.tile(x, (2, 1, 1, 1))), _t(np.tile(s, (2, 1))), _t(np.tile(lab, (2, 1)))).cpu().numpy()
    assert np.isfinite(out).all()
    held(rel_rms(out, g["x0"][:2]), FWD_TOL, FWD_REG, "g5 forward, low-latency class 2")
    assert np.array_equal(one, out[:1]) and np.array_equal(four[:2], out) and np.array_equal(four[2:], out), "class 2 results depend on the batch size"
    with pytest.raises(RuntimeError, match="low-latency class"):
        m(_t(np.tile(x, (3, 1, 1, 1))), _t(np.tile(s, (3, 1))), _t(np.tile(lab, (3, 1))))            # 6 x 256 rows: beyond class 2
    with pytest.raises(ValueError):
        m.set_low_latency(3)


@pytest.mark.parametrize("tag", ["d384", "n1024_d384", "n64_d768", "mlp2_d768"])
def test_low_latency_class_on_other_shapes_vs_golden(tag):
    """The low-latency class away from the 100 M shape, against the reference's own forwards (g16): d = 384 (the finishing kernel's 6-columns-per-lane
    instantiation) at 256 and 1024 tokens, d = 768 at 64 tokens, and mlp_multiplier = 2 (hidden width 1536: four K-splits of 384).  Bit-identical across
    batch sizes inside the class here too."""
    from transformer_latent_diffusion_amd import Denoiser
    g = load_golden("g16_config_sweep.npz")
    cfg = cfg_from_arr(g[f"{tag}_cfg"])
    sd = synth_weights(cfg, g["weight_seed"], g[f"{tag}_checksum"])
    m = Denoiser(**asdict(cfg)).to(_dev()).set_low_latency(True)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    x, s, lab = g[f"{tag}_x"], g[f"{tag}_sigma"], g[f"{tag}_label"]
    out = m(_t(x), _t(s), _t(lab)).cpu().numpy()
    assert np.isfinite(out).all()
    held_key(rel_rms(out, g[f"{tag}_x0"]), FWD_TOL, f"g16_low_latency/{tag}", FWD_REG)
    rep = 2 if tag.startswith("n1024") else 3                      # stays inside the class's 4096 token rows
    big = m(_t(np.tile(x, (rep, 1, 1, 1))), _t(np.tile(s, (rep, 1))), _t(np.tile(lab, (rep, 1)))).cpu().numpy()
    assert np.array_equal(big[:2], out) and np.array_equal(big[-2:], out), tag


def _stress_model(g, tag, env):
    from transformer_latent_diffusion_amd import Denoiser
    cfg = cfg_from_arr(g["cfg"])
    base = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
    sd = dict(base)
    k = str(g["shift_key"])
    sd[k] = (np.asarray(base[k]) + np.float32(g[f"{tag}_shift"])).astype(np.float32)
    old = {kk: os.environ.get(kk) for kk in env}
    os.environ.update(env)
    try:
        m = Denoiser(**asdict(cfg)).to(_dev())
        m.load_state_dict({kk: torch.from_numpy(np.array(v)) for kk, v in sd.items()})
        m.reserve(8)                                 # the fold switches are read when the engine is created
    finally:
        for kk, v in old.items():
            os.environ.pop(kk, None) if v is None else os.environ.__setitem__(kk, v)
    return m


def test_g9_layernorm_stress():
    """Residual rows with a large common offset (g9: |row mean| / row std ~ 4, 28, 85 at block 0).

    The folded LayerNorms take the variance as E[x^2] - E[x]^2 from fp32 partial sums of the STORED bf16 rows
    (LayerNorm-1).  Moderate offsets must meet the forward tolerance.  At 28-85 sigma the bf16 residual
    stream itself is what limits accuracy (a row stored in bf16 keeps ~8 bits below the offset), so there the check
    is that the one-pass statistics add nothing on top: folds on vs the two-pass LayerNorm kernels (folds off)."""
    g = load_golden("g9_ln_stress.npz")
    x, s, lab = _t(g["x"]), _t(g["sigma"]), _t(g["label"])
    report = {}
    for tag in ("mod", "big", "huge"):
        on = _stress_model(g, tag, {})(x, s, lab).cpu().numpy()
        off = _stress_model(g, tag, {"TLD_FOLD_LN1": "0", "TLD_FOLD_LN3": "0"})(x, s, lab).cpu().numpy()
        report[tag] = (rel_rms(on, g[f"{tag}_x0"]), rel_rms(off, g[f"{tag}_x0"]))
    print("g9 rel-rms (folds on, folds off):", report)
    for tag in ("mod", "big", "huge"):
        e_on, e_off = report[tag]
        assert np.isfinite(e_on) and e_on <= FWD_TOL, report            # the reference bound itself, at every offset (measured <= 9.3e-3)
        assert e_on <= 1.5 * e_off + 1e-3, report                       # and the one-pass statistics add nothing over the two-pass kernels


_RANK_SCRIPT = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
from dataclasses import asdict
from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator
from transformer_latent_diffusion_amd.sharded import generate_latents_sharded
from transformer_latent_diffusion_amd.weights import synth_state_dict
dist.init_process_group("gloo")
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = DenoiserConfig(image_size=32, n_channels=4)
m = Denoiser(**asdict(cfg)).to(dev)
m.load_state_dict({{k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 1).items()}})
gen = DiffusionGenerator(m, None, dev, torch.float32)
total = {total}
g = torch.Generator().manual_seed(5)
labels = torch.randn(total, 768, generator=g) * 0.5
out = generate_latents_sharded(gen, labels, n_iter=6, num_imgs=total, class_guidance=4.0, seed=3, img_size=32,
                               sharp_f=0.0, bright_f=0.0)
if dist.get_rank() == 0:
    np.save({out!r}, out.cpu().numpy())
dist.barrier()
dist.destroy_process_group()
"""


@pytest.mark.parametrize("total", [6, 5])
def test_two_ranks_on_one_gpu_match_single_process(total, tmp_path):
    """C2 plumbing on a 1-GPU box: two ranks (both on cuda:0, gloo collectives) each run tld_sample on their slice;
    the all-gathered latents equal the single-process result bit for bit (even and ragged split)."""
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    out = str(tmp_path / "lat.npy")
    script = str(tmp_path / "rank.py")
    open(script, "w").write(_RANK_SCRIPT.format(repo=REPO, tests=TESTS, total=total, out=out))
    port = 29700 + (os.getpid() % 1000) + total
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
                        "127.0.0.1", "--master-port", str(port), script], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.load(out)
    cfg = DenoiserConfig(image_size=32, n_channels=4)
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 1).items()})
    gen = DiffusionGenerator(m, None, _dev(), torch.float32)
    g = torch.Generator().manual_seed(5)
    labels = torch.randn(total, 768, generator=g) * 0.5
    ref = gen.generate_latents(labels, n_iter=6, num_imgs=total, class_guidance=4.0, seed=3, img_size=32, sharp_f=0.0,
                               bright_f=0.0).cpu().numpy()
    assert got.shape == ref.shape and np.array_equal(got, ref)


_RCCL_SCRIPT = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from dataclasses import asdict
from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator
from transformer_latent_diffusion_amd.sharded import generate_latents_sharded
from transformer_latent_diffusion_amd.weights import synth_state_dict
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)       # RCCL communicator on this GPU
cfg = DenoiserConfig(image_size=32, n_channels=4)
m = Denoiser(**asdict(cfg)).to(dev)
m.load_state_dict({{k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 1).items()}})
gen = DiffusionGenerator(m, None, dev, torch.float32)
labels = torch.randn(4, 768, generator=torch.Generator().manual_seed(5)) * 0.5
kw = dict(n_iter=6, num_imgs=4, class_guidance=4.0, seed=3, img_size=32, sharp_f=0.0, bright_f=0.0)
out = generate_latents_sharded(gen, labels, **kw)                           # one all_gather_into_tensor on device memory
ref = gen.generate_latents(labels, **kw)
assert out.is_cuda and torch.equal(out, ref)
dist.barrier(); dist.destroy_process_group()
print("RCCL_OK")
"""


def test_rccl_single_rank_all_gather(tmp_path):
    """The backend the multi-GPU run uses ("nccl" = RCCL) with a one-rank communicator on this GPU: process-group
    creation, the device-memory all_gather_into_tensor of sharded.py and teardown all execute (multi-rank RCCL needs more
    GPUs than this box has; the 2-rank logic is covered by the gloo tests)."""
    script = str(tmp_path / "rccl.py")
    open(script, "w").write(_RCCL_SCRIPT.format(repo=REPO))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29900 + os.getpid() % 500))
    r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "RCCL_OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def test_bench_self_spawns_ranks(tmp_path):
    """`python bench.py --gpus 2` without a launcher re-executes itself under torch.distributed.run (here: both ranks on
    the one GPU, gloo) and prints one JSON line for the 2-rank job; --dump-outputs writes the gathered latents of both ranks."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0",
                        "--same-device", "--backend", "gloo", "--images-per-gpu", "8", "--full", "--no-cpu-baseline",
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=900, env={k: v for k, v in os.environ.items()
                                                                           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["config"]["global_batch"] == 16 and j["value"] > 0 and "roofline" in j
    lat = np.load(tmp_path / "latents.npy")
    assert lat.shape == (16, 4, 32, 32) and lat.dtype == np.float32 and np.isfinite(lat).all()


def test_bench_plain_run_is_headline_only(tmp_path):
    """A plain `bench.py` run times exactly --steps steps and prints the headline line without the --full extras
    (roofline, power, cpu_baseline); --dump-outputs writes the last timed step's latents as float32."""
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--images-per-gpu", "4", "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    j = json.loads(lines[0])
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(j), j
    assert j["steps"] == 2 and j["value"] > 0 and j["ms_per_step"] > 0
    assert not {"roofline", "power", "cpu_baseline"} & set(j), sorted(j)
    lat = np.load(tmp_path / "latents.npy")
    assert lat.shape == (4, 4, 32, 32) and lat.dtype == np.float32 and np.isfinite(lat).all()

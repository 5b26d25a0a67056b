"""CPU: the host side of image-to-image / inpainting -- schedule truncation, the latent-resolution mask, the
argument checks of ``generate_latents_from``, ``sharded_sample``'s per-sample extras, and the CPU reference the GPU tests compare with
(tests/img2img_ref.py), pinned to the oracle loop that g2 pins to the reference."""
import os
import sys
from dataclasses import asdict

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import img2img_ref as R
from conftest import cfg_from_arr, load_golden, synth_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- schedule.truncate_levels --------------------------------------------------------------------------------------------------
def test_truncate_levels_full_strength_keeps_the_schedule():
    from transformer_latent_diffusion_amd import schedule
    full = schedule.noise_schedule(15, 1)
    k, levels = schedule.truncate_levels(full, 1.0)
    assert k == 0 and levels == full and levels[0] == 0.99


def test_truncate_levels_hand_computed():
    """n_iter = 15: levels 0.99, 14/15, 13/15, ... 1/15.  9/15 = 0.6 is the first level <= 0.65 (index 6); 5/15 = 0.333 the first
    <= 0.35 (index 10)."""
    from transformer_latent_diffusion_amd import schedule
    full = schedule.noise_schedule(15, 1)
    k, levels = schedule.truncate_levels(full, 0.65)
    assert k == 6 and levels == full[6:] and len(levels) == 9 and abs(levels[0] - 0.6) < 1e-6
    k, levels = schedule.truncate_levels(full, 0.35)
    assert k == 10 and levels == full[10:] and len(levels) == 5 and abs(levels[0] - 1 / 3) < 1e-6
    # the remaining steps start first-order
    co = schedule.step_coefficients(levels, True)
    assert co[0, 4] == 1.0 and co[0, 5] == 0.0 and co[1, 5] != 0.0


@pytest.mark.parametrize("strength", [0.0, -0.1, 1.0001, 2, float("nan")])
def test_truncate_levels_rejects_strength_outside_unit_interval(strength):
    from transformer_latent_diffusion_amd import schedule
    with pytest.raises(ValueError):
        schedule.truncate_levels(schedule.noise_schedule(15, 1), strength)


@pytest.mark.parametrize("strength", [0.1, 0.05])       # n_iter = 15: only 1/15 = 0.067 is <= 0.1 (one level left); none is <= 0.05
def test_truncate_levels_needs_two_levels(strength):
    from transformer_latent_diffusion_amd import schedule
    with pytest.raises(ValueError):
        schedule.truncate_levels(schedule.noise_schedule(15, 1), strength)


# ---- the CPU reference -----------------------------------------------------------------------------------------------------------
def _tiny_ref():
    from oracle.torch_ref import TorchRefDenoiser
    g = load_golden("g1_tiny32_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    return cfg, TorchRefDenoiser(asdict(cfg), synth_weights(cfg, g["weight_seed"], g["weight_checksum"]))


def _inputs(B=2, S=32, seed=21):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S, S, generator=gen)
    z0 = torch.randn(B, 4, S, S, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


@pytest.mark.parametrize("plus", [True, False])
def test_reference_with_full_schedule_is_the_oracle_sampler(plus):
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    eps, z0, labels = _inputs()
    levels = schedule.noise_schedule(4, 1)
    want = ref.sample(eps, labels, levels, 3.0, plus, 0.1, 0.1)
    got = R.sample_from(ref, eps, z0, None, labels, levels, 1.0, 3.0, plus, 0.1, 0.1)
    assert torch.equal(got, want)


def test_reference_all_ones_mask_is_no_mask():
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    eps, z0, labels = _inputs()
    k, levels = schedule.truncate_levels(schedule.noise_schedule(6, 1), 0.7)
    assert k > 0
    s0 = float(np.float32(levels[0]))
    a = R.sample_from(ref, eps, z0, None, labels, levels, s0, 3.0, True, 0.0, 0.0)
    b = R.sample_from(ref, eps, z0, torch.ones(2, 1, 32, 32), labels, levels, s0, 3.0, True, 0.0, 0.0)
    assert (a == b).all()


def test_reference_keeps_the_known_region_exactly():
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    eps, z0, labels = _inputs()
    k, levels = schedule.truncate_levels(schedule.noise_schedule(6, 1), 0.7)
    s0 = float(np.float32(levels[0]))
    mask = torch.zeros(2, 1, 32, 32)
    mask[0, :, 4:20, 8:30] = 1
    mask[1, :, :, :16] = 1
    out, tx0, txt = R.sample_from(ref, eps, z0, mask, labels, levels, s0, 3.0, True, 0.0, 0.0, trace=True)
    keep = (mask == 0).expand_as(out)
    assert keep.any() and (out[keep] == z0[keep]).all()
    assert not (out[~keep] == z0[~keep]).all()
    for i in range(len(levels) - 1):
        known = levels[i + 1] * eps + (1 - levels[i + 1]) * z0
        assert (txt[i][keep] == known[keep]).all()


# ---- latent_mask -----------------------------------------------------------------------------------------------------------------
def test_latent_mask_area_average():
    from transformer_latent_diffusion_amd import latent_mask
    m = torch.zeros(32, 32)
    m[:8, :8] = 1            # one whole 8 x 8 cell
    m[8:12, 8:16] = 1        # half of the next diagonal cell
    m[31, 31] = 1            # one pixel of the last cell
    out = latent_mask(m, 4)
    want = torch.zeros(1, 4, 4)
    want[0, 0, 0], want[0, 1, 1], want[0, 3, 3] = 1.0, 0.5, 1 / 64
    assert out.shape == (1, 4, 4) and out.dtype == torch.float32 and torch.equal(out, want)
    assert torch.equal(latent_mask(m[None], 4), want)
    from PIL import Image
    pil = Image.fromarray((m.numpy() * 255).astype(np.uint8), mode="L")
    assert torch.equal(latent_mask(pil, 4), want)


def test_latent_mask_rejects_bad_shapes_and_ranges():
    from transformer_latent_diffusion_amd import latent_mask
    with pytest.raises(ValueError):
        latent_mask(torch.zeros(32, 24), 4)                 # not square
    with pytest.raises(ValueError):
        latent_mask(torch.zeros(3, 32, 32), 4)              # three channels
    with pytest.raises(ValueError):
        latent_mask(torch.zeros(30, 30), 4)                 # side not a multiple of the latent size
    with pytest.raises(ValueError):
        latent_mask(torch.full((32, 32), 1.5), 4)
    with pytest.raises(ValueError):
        latent_mask(torch.full((32, 32), -0.1), 4)


# ---- generate_latents_from: host checks come before any device call ---------------------------------------------------------------
class _NoDevice:
    """Stands in for the denoiser: any use of the engine fails the test."""
    n_channels, image_size = 4, 16

    def eval(self):
        raise AssertionError("the model was touched before the host checks finished")

    def sample_latents_from(self, *a, **k):
        raise AssertionError("the sampler was called before the host checks finished")


def test_generate_latents_from_checks_arguments_on_the_host():
    from transformer_latent_diffusion_amd import DiffusionGenerator
    gen = DiffusionGenerator(_NoDevice(), None, torch.device("cpu"), torch.float32)
    z0 = torch.zeros(2, 4, 16, 16)
    lab = torch.zeros(2, 768)
    ok_mask = torch.ones(2, 1, 16, 16)
    with pytest.raises(ValueError):
        gen.generate_latents_from(torch.zeros(2, 4, 16), lab)                                  # not [B,C,S,S]
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, num_imgs=3)                                         # noise batch differs
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, seeds=torch.zeros(2, 4, 32, 32))                    # caller's noise of another size
    with pytest.raises(ValueError):
        gen.generate_latents_from(torch.zeros(2, 3, 16, 16), lab)                              # channels
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, torch.zeros(3, 768))                                     # labels batch
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, mask=torch.ones(2, 4, 16, 16))                      # mask is one channel
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, mask=torch.ones(2, 1, 128, 128))                    # pixel-resolution mask
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, mask=ok_mask * 1.01)
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, mask=ok_mask - 1.5)
    with pytest.raises(ValueError):
        gen.generate_latents_from(z0, lab, mask=ok_mask * float("nan"))
    for strength in (0.0, 1.5, 0.01):
        with pytest.raises(ValueError):
            gen.generate_latents_from(z0, lab, strength=strength, mask=ok_mask, n_iter=15)
    # valid arguments get past the checks and reach the model
    with pytest.raises(AssertionError, match="host checks finished"):
        gen.generate_latents_from(z0, lab, strength=0.6, mask=ok_mask, n_iter=15)


def test_new_names_are_exported():
    import transformer_latent_diffusion_amd as pkg
    for name in ("latent_mask", "generate_latents_from_sharded"):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert hasattr(pkg.Denoiser, "sample_latents_from") and hasattr(pkg.DiffusionGenerator, "generate_from")
    assert hasattr(pkg.DiffusionTransformer, "generate_image_from_image")
    assert "tld_sample_from" in pkg._lib.ABI_SYMBOLS and hasattr(pkg._lib.lib(), "tld_sample_from")


# ---- sharded_sample(extras=...) over gloo, world size 2 ---------------------------------------------------------------------------
def _worker(rank, world, port, total, q):
    sys.path.insert(0, REPO)
    os.environ["OMP_NUM_THREADS"] = "2"
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from transformer_latent_diffusion_amd.sharded import shard_bounds, sharded_sample
        ids = torch.arange(total, dtype=torch.float32)
        x_T = ids.view(total, 1, 1, 1).expand(total, 2, 4, 4).contiguous()
        labels = ids.view(total, 1) * 10
        z0 = ids.view(total, 1, 1, 1).expand(total, 2, 4, 4) * 100
        mask = ids.view(total, 1, 1, 1).expand(total, 1, 4, 4) * 1000
        lo, hi = shard_bounds(total, world, rank)
        seen = {}

        def sample_fn(xs, ls, zs, none, ms):
            assert none is None
            seen["bounds"] = (int(xs[0, 0, 0, 0]), int(xs[-1, 0, 0, 0]) + 1)
            assert zs.shape[0] == ms.shape[0] == ls.shape[0] == xs.shape[0]
            # every extra is this rank's slice of the same samples
            assert torch.equal(zs[:, 0, 0, 0], xs[:, 0, 0, 0] * 100) and torch.equal(ms[:, 0, 0, 0], xs[:, 0, 0, 0] * 1000)
            return xs + ls.view(-1, 1, 1, 1) + zs + ms.expand_as(zs)

        out = sharded_sample(sample_fn, x_T, labels, extras=(z0, None, mask))
        assert seen["bounds"] == (lo, hi)
        if rank == 0:
            q.put(out.numpy())
        dist.barrier()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("total", [4, 5])
def test_sharded_sample_slices_extras_with_x_T(total):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + (os.getpid() % 2000) + total
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    ids = np.arange(total, dtype=np.float32).reshape(total, 1, 1, 1)
    assert np.array_equal(got, np.broadcast_to(ids * 1111, (total, 2, 4, 4)))


def test_sharded_sample_without_a_process_group_passes_extras_through():
    from transformer_latent_diffusion_amd.sharded import sharded_sample
    x, lab, z = torch.zeros(3, 1), torch.zeros(3, 2), torch.ones(3, 1)
    assert torch.equal(sharded_sample(lambda a, b: a + 1, x, lab), x + 1)                      # existing two-argument calls are unchanged
    assert torch.equal(sharded_sample(lambda a, b, c, d: a + c, x, lab, extras=(z, None)), x + 1)
    with pytest.raises(ValueError):
        sharded_sample(lambda a, b, c: a, x, lab, extras=(torch.ones(2, 1),))

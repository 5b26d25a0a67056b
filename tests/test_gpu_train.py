"""GPU: the native training step (tld/train.py:118-175) through the C ABI (tld_train_*).

Oracles: g15 (the reference's own loss.backward() / Adam / EMA on the tiny model, captured by import) and, at the 100 M width, autograd
over the pinned restatement (oracle/torch_ref.train_step_reference) run on the host in the test.
Tolerances (bf16 GEMM operands and saved activations, fp32 accumulation / statistics / optimizer): loss 5e-3 relative, prediction
FWD_TOL (2e-2) rel-rms, every parameter gradient GRAD_TOL = 2e-2 relative L2 -- with one stated exception, tensors whose gradient is
dominated by cancellation noise (norm below 1e-3 of the largest tensor gradient) are held to GRAD_TOL of that largest norm instead."""
import ctypes as C
import os
import subprocess
import sys
from dataclasses import asdict

import numpy as np
import pytest
import torch

from conftest import cfg_from_arr, load_golden, rel_rms, synth_weights
from test_gpu_parity import FWD_TOL, _dev

pytestmark = pytest.mark.gpu

GRAD_TOL = 2e-2
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# Every configuration a test of this file creates a trainer at: name -> (DenoiserConfig arguments, the batch the test steps with, max_batch).  The two golden
# steps (g15 / g17) bring their own configuration.  tests/test_train_plan_host.py sweeps the training step's host plan over this table, on the CPU.
_WIDE = dict(noise_embed_dims=256, patch_size=2, dropout=0, text_emb_size=768, mlp_multiplier=4)
TRAINER_SHAPES = {
    "64 tokens": (dict(image_size=16, n_channels=4, n_layers=1), 16, 16),
    "d192": (dict(image_size=32, n_channels=4, n_layers=2, embed_dim=192), 4, 4),
    "d320": (dict(image_size=32, n_channels=4, n_layers=2, embed_dim=320), 4, 4),
    "4096 tokens": (dict(image_size=128, n_channels=4, n_layers=1), 2, 2),
    "wide": (dict(image_size=32, embed_dim=768, n_layers=2, n_channels=4, **_WIDE), 3, 4),
    "default 2": (dict(image_size=32, n_channels=4), 2, 2),
    "default 4": (dict(image_size=32, n_channels=4), 4, 4),
    "default 8": (dict(image_size=32, n_channels=4), 8, 8),
    "graph d256": (dict(image_size=32, embed_dim=256, n_layers=2, n_channels=4, **_WIDE), 8, 8),
}
GOLDEN_STEPS = ("g15_train_step.npz", "g17_train_step_1024tok.npz")          # (max_batch 4)


def _shape(name):
    from transformer_latent_diffusion_amd import DenoiserConfig
    return DenoiserConfig(**TRAINER_SHAPES[name][0])


def _trainer(cfg, sd, **kw):
    from transformer_latent_diffusion_amd import Trainer
    return Trainer(cfg, device=_dev(), state_dict={k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, **kw)


def _check_grads(got, want, tag):
    norms = {k: float(np.linalg.norm(want[k])) for k in want}
    big = max(norms.values())
    worst = ("", 0.0)
    for k in want:
        err = float(np.linalg.norm(got[k] - want[k]))
        rel = err / max(norms[k], 1e-3 * big)
        if rel > worst[1]:
            worst = (k, rel)
        assert rel <= GRAD_TOL, (tag, k, rel, norms[k], big)
    print(f"{tag}: worst gradient relative L2 {worst[1]:.2e} ({worst[0]})")


def _g15(name="g15_train_step.npz"):
    g = load_golden(name)
    cfg = cfg_from_arr(g["cfg"])
    return g, cfg, synth_weights(cfg, g["weight_seed"], g["weight_checksum"])


@pytest.mark.parametrize("name", list(GOLDEN_STEPS))
def test_forward_backward_vs_reference_step(name):
    """The reference's own training step (loss.backward() on its Denoiser, captured by import): g15 at 256 tokens, g17 at the 512 px
    fine-tuning geometry (image_size 64 = 1024 tokens: two-kernel attention backward, banded depthwise convolution)."""
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    g, cfg, sd = _g15(name)
    tr = _trainer(cfg, sd, max_batch=4)
    x = torch.from_numpy(g["x"])
    xn = mix_noise(x, torch.from_numpy(g["noise_level"]), torch.from_numpy(g["noise"]))
    lab = drop_labels(torch.from_numpy(g["y"]), torch.from_numpy(g["mask"]))
    loss, pred = tr.forward_backward(xn, torch.from_numpy(g["noise_level"]).float(), lab, x)
    assert abs(float(loss) - float(g["loss"])) <= 5e-3 * float(g["loss"]), (float(loss), float(g["loss"]))
    assert rel_rms(pred.cpu().numpy(), g["pred"]) <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: g["grad:" + k] for k in got}, "tiny model vs " + name[:3])
    # bit-reproducible: the same call again leaves the same gradient vector
    first = tr.grads.clone()
    tr.forward_backward(xn, torch.from_numpy(g["noise_level"]).float(), lab, x)
    assert torch.equal(first, tr.grads)


def test_adam_and_ema_kernel_vs_reference_update():
    """The fused optimizer kernel on the REFERENCE's gradients: post-step weights and EMA weights of the fixture (torch.optim.Adam lr 3e-4,
    update_ema alpha 0.999), <= 2e-7 absolute; then a second step against torch.optim.Adam run on the host."""
    g, cfg, sd = _g15()
    from transformer_latent_diffusion_amd import TrainConfig
    tr = _trainer(cfg, sd, max_batch=4, train_cfg=TrainConfig(lr=float(g["lr"]), alpha=float(g["alpha"])))
    host_g = torch.zeros(tr.numel)
    for k, (o, s) in tr.layout.items():
        host_g[o:o + int(np.prod(s))] = torch.from_numpy(g["grad:" + k]).reshape(-1)
    p0 = tr.params.cpu().clone()
    tr.grads.copy_(host_g)
    tr.optimizer_step()
    new, ema = tr.state_dict(), tr.ema_state_dict()
    for k in [k[4:] for k in g if k.startswith("new:")]:
        assert np.abs(new[k].cpu().numpy() - g["new:" + k]).max() <= 2e-7, k
        assert np.abs(ema[k].cpu().numpy() - g["ema:" + k]).max() <= 2e-7, k
    # second step, whole vector, against torch.optim.Adam + the EMA statement on the host
    w = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adam([w], lr=float(g["lr"]))
    e = p0.clone()
    g2 = torch.randn(tr.numel, generator=torch.Generator().manual_seed(4)) * 1e-2
    for gg in (host_g, g2):
        w.grad = gg.clone(); opt.step()
        e.mul_(float(g["alpha"])).add_(w.detach(), alpha=1 - float(g["alpha"]))
    tr.grads.copy_(g2)
    tr.optimizer_step()
    assert (tr.params.cpu() - w.detach()).abs().max() <= 5e-7
    assert (tr.ema.cpu() - e).abs().max() <= 5e-7
    # Adam's bias-correction count follows the optimizer steps; the checkpoint's global_step counts loader iterations (forward_backward calls,
    # tld/train.py:162-174) -- none ran here, the gradients were written directly
    assert tr.step == 2 and tr.checkpoint()["global_step"] == 0


@pytest.mark.parametrize("N", [64, 128, 256, 1024, 4096])
def test_attention_backward_vs_autograd(N):
    """tld_debug_attention_bwd against torch autograd of softmax(q k^T / 8) v on the same bf16-rounded operands: dq, dk, dv <= 2e-2.
    64 / 128 / 256 tokens: one workgroup per (sample, head); 1024: the two-kernel path (row statistics through the scratch vector).
    Asymmetric random operands, so a transposed or mis-ordered fragment cannot cancel."""
    from transformer_latent_diffusion_amd import _lib
    B, H = (3, 2) if N < 4096 else (1, 2)
    d = 64 * H
    gen = torch.Generator().manual_seed(9)
    q, k, v = (torch.randn(B, N, d, generator=gen).bfloat16().float() for _ in range(3))
    q = q * 1.5
    go = torch.randn(B, N, d, generator=gen) * 0.1
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    sp = lambda t: t.view(B, N, H, 64).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(sp(qr), sp(kr), sp(vr)).transpose(1, 2).reshape(B, N, d)
    o.backward(go)
    dev = _dev()
    qk = torch.cat([q, k], dim=-1).bfloat16().to(dev).contiguous()
    vt = v.view(B, N, H, 64).permute(0, 2, 3, 1).contiguous().bfloat16().to(dev)            # [B, H, 64, N]
    ob = o.detach().bfloat16().to(dev).contiguous()
    gd = go.to(dev).contiguous()
    out = torch.zeros(B * N, 3 * d, dtype=torch.bfloat16, device=dev)
    scratch = torch.zeros(2 * B * H * N, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().tld_debug_attention_bwd(C.c_void_p(qk.data_ptr()), C.c_void_p(vt.data_ptr()), C.c_void_p(ob.data_ptr()),
                                                  C.c_void_p(gd.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), B, N, H, st),
               "attention_bwd")
    got = out.float().cpu().view(B, N, 3, d)
    for i, (name, ref) in enumerate((("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad))):
        e = rel_rms(got[:, :, i].numpy(), ref.numpy())
        print(f"attention backward N={N} {name}: rel-rms {e:.2e}")
        assert e <= 2e-2, (name, e)


@pytest.mark.parametrize("rows,n_out,k_in", [(768, 256, 256), (8192, 768, 256), (8384, 512, 768), (16448, 256, 512)])
def test_weight_gradient_gemm_on_untransposed_operands(rows, n_out, k_in):
    """dW = dY^T X on the transposed-operand GEMM (both operands read row-major as the backward left them, fragments through the
    transposing LDS read; split-K over row runs, the last one shorter when rows is not a multiple of the run) against float64 on the
    host: products of bf16 values are exact in fp32, so only the summation order differs -- <= 2e-6 of the result's rms."""
    from transformer_latent_diffusion_amd import _lib
    gen = torch.Generator().manual_seed(rows + n_out)
    dy = (torch.randn(rows, n_out, generator=gen) * 0.3).bfloat16()
    x = (torch.randn(rows, k_in, generator=gen) + 0.25).bfloat16()
    want = dy.double().T @ x.double()
    dev = _dev()
    dyd, xd = dy.to(dev), x.to(dev)
    out = torch.full((n_out, k_in), float("nan"), dtype=torch.float32, device=dev)
    slices = torch.zeros(32 * n_out * k_in, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().tld_debug_wgrad(C.c_void_p(dyd.data_ptr()), C.c_void_p(xd.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(slices.data_ptr()),
                                          slices.numel(), rows, n_out, k_in, st), "wgrad")
    got = out.cpu().double()
    err = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    print(f"weight gradient {rows} x {n_out} x {k_in}: rel-rms {err:.2e}")
    assert err <= 2e-6, err


def test_64_token_step_vs_oracle_autograd():
    """image_size 16 (8 x 8 grid, 64 tokens), one block: every gradient vs autograd over the pinned restatement.  (One block: the test is about
    the 64-token kernels; with two, pos_embed -- the gradient that has passed through every bf16 backward product -- measures 2.1e-2.)"""
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd import DenoiserConfig
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = _shape("64 tokens")
    sd = synth_state_dict(cfg, 41)
    gen = torch.Generator().manual_seed(42)
    B = 16                                   # 1024 token rows, as g15: the tolerance is the one the 256-token goldens hold
    x = torch.randn(B, 4, 16, 16, generator=gen) * 0.8
    y = torch.randn(B, 768, generator=gen) * 0.5
    nl = torch.rand(B, generator=gen, dtype=torch.float64) * 0.9 + 0.05
    noise = torch.randn(B, 4, 16, 16, generator=gen)
    mask = torch.rand(B, generator=gen) < 0.25
    loss_ref, pred_ref, grads_ref = train_step_reference(cfg, sd, x, nl, noise, y, mask)
    tr = _trainer(cfg, sd, max_batch=16)
    loss, pred = tr.forward_backward(mix_noise(x, nl, noise), nl.float(), drop_labels(y, mask), x)
    assert abs(float(loss) - loss_ref) <= 5e-3 * loss_ref, (float(loss), loss_ref)
    assert rel_rms(pred.cpu().numpy(), pred_ref.numpy()) <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: grads_ref[k].numpy() for k in got}, "64-token model vs oracle autograd")


@pytest.mark.parametrize("d", [192, 320])
def test_odd_width_step_vs_oracle_autograd(d):
    """embed_dim a multiple of 64 that is not one of 128 (3 / 5 heads; the reference's own domain, transformer_blocks.py:126-128): 128-wide GEMM tiles
    with partial last tiles, the transposing weight-gradient path, 2-byte row kernels; every gradient vs autograd over the pinned restatement."""
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd import DenoiserConfig
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = _shape(f"d{d}")
    sd = synth_state_dict(cfg, 45 + d)
    gen = torch.Generator().manual_seed(46)
    B = 4
    x = torch.randn(B, 4, 32, 32, generator=gen) * 0.8
    y = torch.randn(B, 768, generator=gen) * 0.5
    nl = torch.tensor([0.1, 0.35, 0.6, 0.85], dtype=torch.float64)
    noise = torch.randn(B, 4, 32, 32, generator=gen)
    mask = torch.tensor([False, False, True, False])
    loss_ref, pred_ref, grads_ref = train_step_reference(cfg, sd, x, nl, noise, y, mask)
    tr = _trainer(cfg, sd, max_batch=4)
    loss, pred = tr.forward_backward(mix_noise(x, nl, noise), nl.float(), drop_labels(y, mask), x)
    assert abs(float(loss) - loss_ref) <= 5e-3 * loss_ref, (float(loss), loss_ref)
    assert rel_rms(pred.cpu().numpy(), pred_ref.numpy()) <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: grads_ref[k].numpy() for k in got}, f"d = {d} model vs oracle autograd")


def test_4096_token_step_vs_oracle_autograd():
    """image_size 128 (64 x 64 grid, 4096 tokens: the 1024 px fine-tuning geometry), one block, two samples: 16 query / key blocks in the two-kernel
    attention backward, four row bands in the depthwise convolution; every gradient vs autograd over the pinned restatement."""
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd import DenoiserConfig
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = _shape("4096 tokens")
    sd = synth_state_dict(cfg, 43)
    gen = torch.Generator().manual_seed(44)
    B = 2
    x = torch.randn(B, 4, 128, 128, generator=gen) * 0.8
    y = torch.randn(B, 768, generator=gen) * 0.5
    nl = torch.tensor([0.2, 0.7], dtype=torch.float64)
    noise = torch.randn(B, 4, 128, 128, generator=gen)
    mask = torch.tensor([False, True])
    loss_ref, pred_ref, grads_ref = train_step_reference(cfg, sd, x, nl, noise, y, mask)
    tr = _trainer(cfg, sd, max_batch=2)
    loss, pred = tr.forward_backward(mix_noise(x, nl, noise), nl.float(), drop_labels(y, mask), x)
    assert abs(float(loss) - loss_ref) <= 5e-3 * loss_ref, (float(loss), loss_ref)
    assert rel_rms(pred.cpu().numpy(), pred_ref.numpy()) <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: grads_ref[k].numpy() for k in got}, "4096-token model vs oracle autograd")


def test_wide_model_gradients_vs_oracle_autograd():
    """100 M-class width (d = 768, 12 heads, hidden 3072), 2 blocks, B = 3: every gradient vs autograd over the pinned restatement."""
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd import DenoiserConfig
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = _shape("wide")
    sd = synth_state_dict(cfg, 31)
    gen = torch.Generator().manual_seed(32)
    B = 3
    x = torch.randn(B, 4, 32, 32, generator=gen) * 0.8
    y = torch.randn(B, 768, generator=gen) * 0.5
    nl = torch.tensor([0.07, 0.45, 0.9], dtype=torch.float64)
    noise = torch.randn(B, 4, 32, 32, generator=gen)
    mask = torch.tensor([False, False, True])
    loss_ref, pred_ref, grads_ref = train_step_reference(cfg, sd, x, nl, noise, y, mask)
    tr = _trainer(cfg, sd, max_batch=4)
    loss, pred = tr.forward_backward(mix_noise(x, nl, noise), nl.float(), drop_labels(y, mask), x)
    assert abs(float(loss) - loss_ref) <= 5e-3 * loss_ref, (float(loss), loss_ref)
    assert rel_rms(pred.cpu().numpy(), pred_ref.numpy()) <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: grads_ref[k].numpy() for k in got}, "d = 768, 2 blocks vs oracle autograd")


def test_training_reduces_the_loss_and_ema_loads_into_the_inference_engine():
    """A few steps of Trainer.train_step on a fixed batch: the loss goes down; the EMA state_dict loads into the inference Denoiser."""
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, TrainConfig, Trainer
    cfg = _shape("default 4")
    tr = Trainer(cfg, TrainConfig(lr=1e-3, alpha=0.9), device=_dev(), init_seed=2, max_batch=8)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(8, 4, 32, 32, generator=gen) * 0.8
    y = torch.randn(8, 768, generator=gen) * 0.5
    losses = []
    for i in range(12):
        rng, tg = np.random.default_rng(0), torch.Generator().manual_seed(0)          # the same noise every step: a fixed objective
        losses.append(float(tr.train_step(x, y, np_rng=rng, generator=tg)))
    assert all(np.isfinite(losses)) and losses[-1] < 0.7 * losses[0], losses
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict(tr.ema_state_dict())
    out = m(x[:2].to(_dev()), torch.full((2, 1), 0.5, device=_dev()), y[:2].to(_dev()))
    assert out.shape == (2, 4, 32, 32) and torch.isfinite(out).all()


_RANK = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from transformer_latent_diffusion_amd import DenoiserConfig, TrainConfig, Trainer
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = DenoiserConfig(image_size=32, n_channels=4)
tr = Trainer(cfg, TrainConfig(lr=3e-4), device=dev, init_seed=3, max_batch=4)
g = torch.Generator().manual_seed(7)
x = torch.randn(4, 4, 32, 32, generator=g) * 0.8; y = torch.randn(4, 768, generator=g) * 0.5
nl = torch.tensor([0.1, 0.3, 0.6, 0.8]); noise = torch.randn(4, 4, 32, 32, generator=g)
xn = nl.view(-1, 1, 1, 1) * noise + (1 - nl.view(-1, 1, 1, 1)) * x
sl = slice(r * 4 // w, (r + 1) * 4 // w)
tr.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
# gloo moves device tensors through the host; RCCL ("nccl") is what a multi-GPU node uses -- same call
if w > 1:
    # overlapped reduction (default): one asynchronous all-reduce per decoder block, last block first, then the two ranges around the blocks;
    # together they tile the flat gradient vector exactly once
    sl_ = sorted(tr._slices)
    assert len(tr._slices) == cfg.n_layers + 2 and len(tr._pending) == cfg.n_layers + 2, tr._slices
    assert sl_[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(sl_, sl_[1:])) and sl_[-1][0] + sl_[-1][1] == tr.numel, sl_
    first_blocks = [o for o, n in tr._slices[:cfg.n_layers]]
    assert first_blocks == sorted(first_blocks, reverse=True), first_blocks
tr.optimizer_step()
if w > 1:
    # the same step with ONE blocking all-reduce after the backward (overlap_allreduce=False) lands on the same parameters, bit for bit
    tr2 = Trainer(cfg, TrainConfig(lr=3e-4), device=dev, init_seed=3, max_batch=4, overlap_allreduce=False)
    tr2.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
    assert not tr2._pending
    tr2.optimizer_step()
    torch.cuda.synchronize()
    assert torch.equal(tr.params, tr2.params), float((tr.params - tr2.params).abs().max())
    # a second forward_backward without an optimizer step in between drains the first call's reductions before the backward rewrites the
    # gradients, and grad_dict() hands out the fully reduced SUM
    tr.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
    tr.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
    gsum = torch.cat([v.reshape(-1) for v in tr.grad_dict().values()]).clone()
    assert not tr._pending
    tr2.forward_backward(xn[sl], nl[sl], y[sl], x[sl]); dist.all_reduce(tr2.grads)
    torch.cuda.synchronize()
    assert torch.equal(gsum, tr2.grads)
    tr.optimizer_step()
    # an exception inside the gradient-ready callback (ctypes would swallow it) surfaces from forward_backward, on every rank alike, and the
    # optimizer then refuses nothing silently: the next optimizer_step falls back to the blocking all-reduce of the whole vector
    real, calls = dist.all_reduce, [0]
    def flaky(*a, **k):
        calls[0] += 1
        if calls[0] == 3:
            raise RuntimeError("injected collective failure")
        return real(*a, **k)
    dist.all_reduce = flaky
    try:
        tr.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
        raise SystemExit("the injected failure did not surface")
    except RuntimeError as e:
        assert "all-reduce of a slice failed" in str(e) and "injected" in str(e.__cause__), e
    finally:
        dist.all_reduce = real
    assert not tr._pending and not tr._reduced and len(tr._slices) == 2
    # partly recorded slices never reach the 1 / world path
    tr._reduced = True
    try:
        tr.optimizer_step()
        raise SystemExit("stepped on partly reduced gradients")
    except RuntimeError as e:
        assert "partly reduced" in str(e), e
torch.save(tr.params.cpu() if w == 1 else tr2.params.cpu(), {out!r} + f".{{w}}.{{r}}")
print("rank", r, "done")
"""


def test_two_ranks_average_gradients_like_one_process(tmp_path):
    """DDP semantics of the step: two ranks (both on this GPU, gloo collectives) each take half of a batch; after the all-reduce + Adam
    step both hold the same parameters, and those equal a single process stepping on the whole batch (the loss is a mean over equally
    sized shards) up to summation order."""
    script = tmp_path / "rank.py"
    out = str(tmp_path / "params")
    script.write_text(_RANK.format(repo=REPO, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for w in (2, 1):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={w}", "--master-addr", "127.0.0.1",
                            "--master-port", "29563", str(script)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b, one = torch.load(out + ".2.0"), torch.load(out + ".2.1"), torch.load(out + ".1.0")
    assert torch.equal(a, b)
    # Adam's first step moves every weight by ~lr * sign(g): compare the UPDATE directions where the gradient is not at noise level
    base = torch.cat([torch.from_numpy(np.array(v)).reshape(-1) for k, v in __import__("transformer_latent_diffusion_amd").weights.synth_state_dict(
        __import__("transformer_latent_diffusion_amd").DenoiserConfig(image_size=32, n_channels=4), 3).items()
        if "angular" not in k and "precomputed" not in k])
    da, d1 = a - base, one - base
    agree = (torch.sign(da) == torch.sign(d1)).float().mean().item()
    assert agree > 0.97, agree
    assert (da - d1).abs().max() <= 2 * 3e-4 + 1e-7


def test_graph_replay_equals_eager_steps(monkeypatch):
    """TLD_TRAIN_GRAPH=1: forward + backward captured into a HIP graph on the second full-batch step and replayed from fixed buffers.
    Five optimizer steps give bit-identical losses and parameters to the eager path."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("graph d256")

    def run(graph):
        monkeypatch.setenv("TLD_TRAIN_GRAPH", "1" if graph else "0")
        tr = Trainer(cfg, TrainConfig(batch_size=8), device="cuda:0", init_seed=3, max_batch=8)
        g = torch.Generator().manual_seed(5)
        rng = np.random.default_rng(7)
        losses = []
        for _ in range(5):
            x = torch.randn(8, 4, 32, 32, generator=g)
            y = torch.randn(8, 768, generator=g)
            losses.append(float(tr.train_step(x, y, np_rng=rng, generator=g)))
        torch.cuda.synchronize()
        return losses, tr.params.clone(), tr._graph is not None

    l0, p0, g0 = run(False)
    l1, p1, g1 = run(True)
    assert not g0 and g1
    assert l0 == l1 and torch.equal(p0, p1)


def test_graph_capture_refreshes_weights_and_pred_is_not_aliased(monkeypatch):
    """two forward_backward calls in a row (gradient accumulation / reproducibility checks) make the capture happen with the engine's
    weights_fresh flag SET; the refresh kernels must still be part of the graph, or every replay after an Adam step runs on stale bf16 weights.
    Sequence fb, fb (captures), step, fb, step, fb in graph mode == the same sequence eagerly, bit for bit; returned predictions are copies."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("graph d256")

    def run(graph):
        monkeypatch.setenv("TLD_TRAIN_GRAPH", "1" if graph else "0")
        tr = Trainer(cfg, TrainConfig(batch_size=8), device="cuda:0", init_seed=3, max_batch=8)
        g = torch.Generator().manual_seed(9)
        batches = [(torch.randn(8, 4, 32, 32, generator=g), torch.rand(8, generator=g) * 0.9 + 0.05, torch.randn(8, 768, generator=g),
                    torch.randn(8, 4, 32, 32, generator=g)) for _ in range(4)]
        out = []
        l, p = tr.forward_backward(*batches[0]); out.append((float(l), p))
        l, p = tr.forward_backward(*batches[1]); out.append((float(l), p))        # second full-batch call: capture in graph mode
        tr.optimizer_step()
        l, p = tr.forward_backward(*batches[2]); out.append((float(l), p))
        tr.optimizer_step()
        l, p = tr.forward_backward(*batches[3]); out.append((float(l), p))
        torch.cuda.synchronize()
        return out, tr.grads.clone(), tr._graph is not None

    e, ge, g0 = run(False)
    r, gr, g1 = run(True)
    assert not g0 and g1
    for (le, pe), (lr, pr) in zip(e, r):
        assert le == lr and torch.equal(pe, pr)
    assert torch.equal(ge, gr)
    assert r[1][1].data_ptr() != r[2][1].data_ptr() and not torch.equal(r[1][1], r[2][1])      # replays hand out copies


def test_checkpoint_is_reference_format_and_resumes(tmp_path):
    """The checkpoint dict is the reference's (tld/train.py:150-156): model_ema, torch.optim.Adam's state_dict layout, global_step -- and
    Trainer.load_checkpoint resumes from it (tld/train.py:92-104): a run continued from the checkpoint takes the same steps as the original."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("default 4")
    tr = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=1, max_batch=4)
    g = torch.Generator().manual_seed(2); rng = np.random.default_rng(3)
    for _ in range(3):
        tr.train_step(torch.randn(4, 4, 32, 32, generator=g), torch.randn(4, 768, generator=g), np_rng=rng, generator=g)
    ck = tr.checkpoint()
    assert set(ck) == {"model_ema", "opt_state", "global_step"} and ck["global_step"] == 3
    osd = ck["opt_state"]
    # torch.optim.Adam accepts it for a parameter list of the same shapes
    ps = [torch.nn.Parameter(torch.zeros(s)) for _, s in tr.layout.values()]
    opt = torch.optim.Adam(ps, lr=1e-3)
    opt.load_state_dict(osd)
    assert float(opt.state[ps[0]]["step"]) == 3.0 and opt.param_groups[0]["lr"] == tr.tc.lr
    path = str(tmp_path / "ck.pth")
    torch.save(ck, path)
    # resume: the reference loads the EMA weights into the live model -- do the same to the original, then both continue identically
    tr.load_checkpoint(ck)
    tr2 = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=99, max_batch=4).load_checkpoint(path)
    assert tr2.step == 3 and torch.equal(tr2.params, tr.params) and torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq)
    x, y = torch.randn(4, 4, 32, 32, generator=g), torch.randn(4, 768, generator=g)
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    l1 = tr.train_step(x, y, np_rng=np.random.default_rng(8), generator=g1)
    l2 = tr2.train_step(x, y, np_rng=np.random.default_rng(8), generator=g2)
    assert float(l1) == float(l2) and torch.equal(tr.params, tr2.params) and tr2.step == 4 and tr2.global_step == 4
    # a checkpoint without optimizer state (saved before the first step of a run that had itself resumed): the loop counter comes back, Adam's
    # bias-correction count stays 0 with its zero moments -- torch.optim.Adam does the same with an empty state
    tr3 = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=99, max_batch=4)
    tr3.load_checkpoint({"model_ema": ck["model_ema"], "opt_state": {"state": {}, "param_groups": ck["opt_state"]["param_groups"]}, "global_step": 1000})
    assert tr3.step == 0 and tr3.global_step == 1000 and tr3.checkpoint()["global_step"] == 1000
    tr3.optimizer_step()
    assert tr3.step == 1 and tr3.global_step == 1000           # (the loop counter counts forward_backward calls -- loader iterations -- not optimizer steps)


def test_gradient_accumulation_equals_one_large_batch():
    """accelerator.accumulate() with gradient_accumulation_steps = 2 (tld/train.py:160): two micro-batches of 4 folded with ``last_micro_batch=False`` /
    default step on the mean of their gradients = the gradient of the mean loss over all 8 samples, i.e. what ONE batch of 8 gives (up to the
    summation order of the weight-gradient reductions), and the optimizer lands on the same parameters."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("default 4")
    g = torch.Generator().manual_seed(4)
    x = torch.randn(8, 4, 32, 32, generator=g) * 0.8; y = torch.randn(8, 768, generator=g) * 0.5
    nl = torch.rand(8, generator=g) * 0.9 + 0.05; noise = torch.randn(8, 4, 32, 32, generator=g)
    xn = nl.view(-1, 1, 1, 1) * noise + (1 - nl.view(-1, 1, 1, 1)) * x
    one = Trainer(cfg, TrainConfig(batch_size=8), device="cuda:0", init_seed=6, max_batch=8, use_graph=False)
    l_one, _ = one.forward_backward(xn, nl, y, x)
    g_one = one.grads.clone()
    acc = Trainer(cfg, TrainConfig(batch_size=8), device="cuda:0", init_seed=6, max_batch=8, use_graph=False)
    la, _ = acc.forward_backward(xn[:4], nl[:4], y[:4], x[:4], last_micro_batch=False)
    with pytest.raises(RuntimeError, match="middle of a gradient accumulation"):
        acc.optimizer_step()
    lb, _ = acc.forward_backward(xn[4:], nl[4:], y[4:], x[4:])
    assert abs(0.5 * (float(la) + float(lb)) - float(l_one)) <= 1e-5 * abs(float(l_one)) + 1e-7
    g_acc = acc.grads * acc._micro_scale                       # optimizer_step applies the 1 / 2
    rel = float((g_acc - g_one).norm() / g_one.norm())
    assert rel <= 1e-5, rel                                    # bf16 operands are the same per sample; only fp32 summation orders differ (measured 6e-8)
    one.optimizer_step(); acc.optimizer_step()
    assert acc._acc_n == 0 and acc._micro_scale == 1.0 and acc.step == 1
    assert one.global_step == 1 and acc.global_step == 2       # the loop counter counts micro-batches (tld/train.py:162-174), Adam's count optimizer steps
    d = float((acc.params - one.params).abs().max())
    assert d <= 0.1 * one.tc.lr, d                             # Adam's first step is lr * g / (|g| + eps): differs only where |g| is at the 1e-8 eps level (measured 0.007 lr)
    frac = float(((acc.params - one.params).abs() > 1e-6).float().mean())
    assert frac <= 1e-3, frac                                  # (measured 1e-6)


def test_abandoned_accumulation_can_be_reset_and_explicit_use_graph_beats_the_environment(monkeypatch):
    """(a) a step abandoned in the middle of an accumulation must not poison the next one -- reset_accumulation() drops the folded
    gradients (load_state_dict does it too); (b) an explicit use_graph= argument wins over TLD_TRAIN_GRAPH."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("default 4")
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4, 4, 32, 32, generator=g) * 0.8; y = torch.randn(4, 768, generator=g) * 0.5
    nl = torch.rand(4, generator=g) * 0.9 + 0.05; noise = torch.randn(4, 4, 32, 32, generator=g)
    xn = nl.view(-1, 1, 1, 1) * noise + (1 - nl.view(-1, 1, 1, 1)) * x
    monkeypatch.setenv("TLD_TRAIN_GRAPH", "1")
    ref = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=6, max_batch=4, use_graph=False)
    assert ref.use_graph is False
    monkeypatch.delenv("TLD_TRAIN_GRAPH")
    ref.forward_backward(xn, nl, y, x)
    g_ref = ref.grads.clone()
    tr = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=6, max_batch=4, use_graph=False)
    tr.forward_backward(xn.flip(0), nl.flip(0), y.flip(0), x.flip(0), last_micro_batch=False)      # ... and the step is abandoned here
    with pytest.raises(RuntimeError, match="reset_accumulation"):
        tr.optimizer_step()
    tr.reset_accumulation()
    assert tr._acc_n == 0 and tr._micro_scale == 1.0 and float(tr._acc.abs().max()) == 0.0
    tr.forward_backward(xn, nl, y, x)
    assert torch.equal(tr.grads, g_ref)                       # nothing of the abandoned micro-batch is left in the gradients
    tr.optimizer_step()
    assert tr.step == 1 and tr.global_step == 2
    tr.forward_backward(xn, nl, y, x, last_micro_batch=False)
    tr.load_state_dict(ref.state_dict())
    assert tr._acc_n == 0


def test_gradient_accumulation_under_graph_replay_and_ragged_staging():
    """Accumulation with the forward + backward replayed from the HIP graph (full micro-batches) lands on the parameters of the eager path, step after step;
    and train_step's pinned staging follows a batch whose size changes (the last, smaller batch of an epoch) and changes back."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("default 4")
    g = torch.Generator().manual_seed(12)
    mk = lambda n: (torch.randn(n, 4, 32, 32, generator=g) * 0.8, torch.rand(n, generator=g) * 0.9 + 0.05, torch.randn(n, 768, generator=g) * 0.5,
                    torch.randn(n, 4, 32, 32, generator=g))
    batches = [mk(4) for _ in range(6)]
    res = {}
    for graph in (True, False):
        tr = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=4, max_batch=4, use_graph=graph)
        for i in range(0, 6, 2):
            tr.forward_backward(*batches[i], last_micro_batch=False)
            tr.forward_backward(*batches[i + 1])
            tr.optimizer_step()
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph and tr.step == 3
        res[graph] = tr.params.clone()
    assert torch.equal(res[True], res[False])
    a = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=4, max_batch=4)
    b = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=4, max_batch=4, use_graph=False)
    x, y = torch.randn(4, 4, 32, 32, generator=g) * 0.8, torch.randn(4, 768, generator=g) * 0.5
    for i, n in enumerate((4, 4, 3, 4, 2, 4)):
        la = a.train_step(x[:n], y[:n], np_rng=np.random.default_rng(i), generator=torch.Generator().manual_seed(i))
        xn, nl, lab = b.make_batch(x[:n], y[:n], np.random.default_rng(i), torch.Generator().manual_seed(i))
        lb, _ = b.forward_backward(xn.cuda(), nl.cuda(), lab.cuda(), x[:n].cuda())
        b.optimizer_step()
        assert float(la) == float(lb), (i, n, float(la), float(lb))
    torch.cuda.synchronize()
    assert torch.equal(a.params, b.params)


def test_train_step_stages_host_batches_without_blocking_and_matches_device_batches():
    """train_step on HOST tensors goes through pinned double buffers and a copy stream (round 5); the result equals forward_backward + optimizer_step
    on the same batch handed over as device tensors, step after step (graph replay on and off)."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = _shape("default 4")
    g = torch.Generator().manual_seed(8)
    x = torch.randn(4, 4, 32, 32, generator=g) * 0.8; y = torch.randn(4, 768, generator=g) * 0.5
    for graph in (True, False):
        a = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=2, max_batch=4, use_graph=graph)
        b = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=2, max_batch=4, use_graph=False)
        assert a.use_graph == graph
        for i in range(4):
            la = a.train_step(x, y, np_rng=np.random.default_rng(i), generator=torch.Generator().manual_seed(i))
            xn, nl, lab = b.make_batch(x, y, np.random.default_rng(i), torch.Generator().manual_seed(i))
            lb, _ = b.forward_backward(xn.cuda(), nl.cuda(), lab.cuda(), x.cuda())
            b.optimizer_step()
            assert float(la) == float(lb), (graph, i, float(la), float(lb))
        torch.cuda.synchronize()
        assert torch.equal(a.params, b.params), graph


def test_trainer_refuses_dropout_and_resolves_current_device():
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    with pytest.raises(NotImplementedError):
        Trainer(DenoiserConfig(image_size=32, n_channels=4, dropout=0.1), device="cuda:0")
    tr = Trainer(DenoiserConfig(image_size=32, n_channels=4), device="cuda", max_batch=2)
    assert tr.device == torch.device("cuda", torch.cuda.current_device()) and tr.params.device == tr.device

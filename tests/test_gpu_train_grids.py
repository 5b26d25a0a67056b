"""Training at every latent grid the inference engine serves (G x G tokens, G a multiple of 4, 4 <= G <= 64), not only at the five token
counts whose attention backward tiles exactly (64, 256, 1024, 2304, 4096).

The attention backward alone against torch autograd at token counts that are not multiples of its block (partial last block, and at
N % 32 == 16 a half-empty 32 x 32 tile); whole training steps against autograd over the pinned restatement at G = 4, 12, 20, 24, 36, 44, 60 and the
100 M width; graph replay against eager steps; the fine-tuning workflow from a 32-latent model to 48; the edges of the domain.
Tolerances are those of tests/test_gpu_train.py: loss 5e-3 relative, prediction FWD_TOL rel-rms, gradients GRAD_TOL relative L2."""
import ctypes as C
from dataclasses import asdict, replace

import numpy as np
import pytest
import torch

from conftest import rel_rms
from test_gpu_parity import FWD_TOL, _dev
from test_gpu_train import _check_grads, _trainer

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("N", [16, 144, 400, 576, 784, 1600, 3136])
def test_attention_backward_any_token_count_vs_autograd(N):
    """tld_debug_attention_bwd at token counts that are multiples of 16 but not of the kernel's block: dq, dk, dv <= 2e-2 rel-rms against
    autograd on the same bf16-rounded operands (asymmetric operands, q scaled by 1.5), every value finite, the last (sample, head) on its
    own, and nothing written past the B N output rows or the 2 B H N statistics floats (sentinels one block beyond both)."""
    from transformer_latent_diffusion_amd import _lib
    B, H = (3, 2) if N <= 1600 else (1, 2)
    d = 64 * H
    gen = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(B, N, d, generator=gen).bfloat16().float() for _ in range(3))
    q = q * 1.5
    go = torch.randn(B, N, d, generator=gen) * 0.1
    qr, kr, vr = (t.clone().requires_grad_(True) for t in (q, k, v))
    sp = lambda t: t.view(B, N, H, 64).transpose(1, 2)
    o = torch.nn.functional.scaled_dot_product_attention(sp(qr), sp(kr), sp(vr)).transpose(1, 2).reshape(B, N, d)
    o.backward(go)
    dev = _dev()
    qk = torch.cat([q, k], dim=-1).bfloat16().to(dev).contiguous()
    vt = v.view(B, N, H, 64).permute(0, 2, 3, 1).contiguous().bfloat16().to(dev)
    ob = o.detach().bfloat16().to(dev).contiguous()
    gd = go.to(dev).contiguous()
    SENT = 1024.0                                   # exact in bf16 and fp32
    pad = 256                                       # the widest block
    out = torch.full((B * N + pad, 3 * d), SENT, dtype=torch.bfloat16, device=dev)
    scratch = torch.full((2 * B * H * N + 2 * pad,), SENT, dtype=torch.float32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().tld_debug_attention_bwd(C.c_void_p(qk.data_ptr()), C.c_void_p(vt.data_ptr()), C.c_void_p(ob.data_ptr()),
                                                  C.c_void_p(gd.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), B, N, H, st),
               "attention_bwd")
    torch.cuda.synchronize()
    tail = out[B * N:].float().cpu()
    assert bool((tail == SENT).all()), f"N={N}: {int((tail != SENT).sum())} values written past row B N"
    assert bool((scratch[2 * B * H * N:].cpu() == SENT).all()), f"N={N}: statistics written past 2 B H N"
    got = out[:B * N].float().cpu().view(B, N, 3, d)
    assert bool(torch.isfinite(got).all()), f"N={N}: non-finite gradient"
    for i, (name, ref) in enumerate((("dq", qr.grad), ("dk", kr.grad), ("dv", vr.grad))):
        e = rel_rms(got[:, :, i].numpy(), ref.numpy())
        e_last = rel_rms(got[B - 1, :, i, d - 64:].numpy(), ref[B - 1, :, d - 64:].numpy())
        print(f"attention backward N={N} {name}: rel-rms {e:.2e}, last (sample, head) {e_last:.2e} (bound 2e-2)")
        assert e <= 2e-2 and e_last <= 2e-2, (name, e, e_last)


def _step_vs_oracle(cfg, B, seed, tag):
    from oracle.torch_ref import train_step_reference
    from transformer_latent_diffusion_amd.train import drop_labels, mix_noise
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    S = cfg.image_size
    sd = synth_state_dict(cfg, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, 4, S, S, generator=gen) * 0.8
    y = torch.randn(B, 768, generator=gen) * 0.5
    nl = torch.rand(B, generator=gen, dtype=torch.float64) * 0.9 + 0.05
    noise = torch.randn(B, 4, S, S, generator=gen)
    mask = torch.arange(B) % 3 == 1
    loss_ref, pred_ref, grads_ref = train_step_reference(cfg, sd, x, nl, noise, y, mask)
    tr = _trainer(cfg, sd, max_batch=B)
    loss, pred = tr.forward_backward(mix_noise(x, nl, noise), nl.float(), drop_labels(y, mask), x)
    rl, rp = abs(float(loss) - loss_ref) / loss_ref, rel_rms(pred.cpu().numpy(), pred_ref.numpy())
    print(f"{tag}: loss rel {rl:.2e} (bound 5e-3), prediction rel-rms {rp:.2e} (bound {FWD_TOL})")
    assert rl <= 5e-3, (float(loss), loss_ref)
    assert rp <= FWD_TOL
    got = {k: v.cpu().numpy() for k, v in tr.grad_dict().items()}
    _check_grads(got, {k: grads_ref[k].numpy() for k in got}, tag)


# image_size 8: G = 4, 16 tokens (one 32-token block, half of it masked); 24: G = 12, 144 tokens (single-workgroup attention backward, the
# three-kernel depthwise backward); 40: G = 20, 400 tokens (two-kernel path, a half-empty 32-token tile); 48: G = 24, 576 tokens (384 px).
# The batches leave B N off a multiple of 64 rows at G = 4, 12 and 20 (the padded weight-gradient contraction).
# 72, 88, 120: G = 36, 44, 60 (1296, 1936, 3600 tokens): the 6- and 8-wave masked kernel pairs of the attention backward.
@pytest.mark.parametrize("image_size,B", [(8, 7), (24, 5), (40, 3), (48, 2), (72, 2), (88, 1), (120, 1)])
def test_new_grid_step_vs_oracle_autograd(image_size, B):
    from transformer_latent_diffusion_amd import DenoiserConfig
    cfg = DenoiserConfig(image_size=image_size, n_channels=4, n_layers=1)
    G = image_size // 2
    _step_vs_oracle(cfg, B, 60 + image_size, f"G = {G} ({G * G} tokens), B = {B} vs oracle autograd")


def test_576_token_wide_model_vs_oracle_autograd():
    """The 100 M width (d = 768, 12 heads) at the 384 px grid, two blocks."""
    from transformer_latent_diffusion_amd import DenoiserConfig
    cfg = DenoiserConfig(image_size=48, noise_embed_dims=256, patch_size=2, embed_dim=768, dropout=0, n_layers=2, text_emb_size=768, n_channels=4,
                         mlp_multiplier=4)
    _step_vs_oracle(cfg, 2, 71, "d = 768, 2 blocks, 576 tokens vs oracle autograd")


def test_576_token_graph_replay_equals_eager_steps(monkeypatch):
    """The step at 576 tokens captured into a HIP graph and replayed: five optimizer steps bit-identical to the eager path."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    from transformer_latent_diffusion_amd.train import TrainConfig
    cfg = DenoiserConfig(image_size=48, noise_embed_dims=256, patch_size=2, embed_dim=256, dropout=0, n_layers=2, text_emb_size=768, n_channels=4,
                         mlp_multiplier=4)

    def run(graph):
        monkeypatch.setenv("TLD_TRAIN_GRAPH", "1" if graph else "0")
        tr = Trainer(cfg, TrainConfig(batch_size=4), device="cuda:0", init_seed=3, max_batch=4)
        g = torch.Generator().manual_seed(5)
        rng = np.random.default_rng(7)
        losses = []
        for _ in range(5):
            x = torch.randn(4, 4, 48, 48, generator=g)
            y = torch.randn(4, 768, generator=g)
            losses.append(float(tr.train_step(x, y, np_rng=rng, generator=g)))
        torch.cuda.synchronize()
        return losses, tr.params.clone(), tr._graph is not None

    l0, p0, g0 = run(False)
    l1, p1, g1 = run(True)
    assert not g0 and g1
    assert l0 == l1 and torch.equal(p0, p1)


def test_fine_tune_from_32_to_48_latents():
    """A model built at image_size 32, its position table resampled to 48 (upsample_pos_embed), trained a few steps at 576 tokens: the loss
    falls; the checkpoint round-trips through load_checkpoint; the EMA weights load into the inference Denoiser(image_size=48), whose forward
    matches the restatement on the same weights within FWD_TOL."""
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, TrainConfig, Trainer
    from transformer_latent_diffusion_amd.checkpoint import upsample_pos_embed
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg32 = DenoiserConfig(image_size=32, n_channels=4, n_layers=2)
    sd48 = upsample_pos_embed({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg32, 81).items()}, 48)
    cfg = replace(cfg32, image_size=48)
    tc = TrainConfig(lr=1e-3, alpha=0.9)
    tr = Trainer(cfg, tc, device=_dev(), state_dict=sd48, max_batch=4)
    gen = torch.Generator().manual_seed(82)
    x = torch.randn(4, 4, 48, 48, generator=gen) * 0.8
    y = torch.randn(4, 768, generator=gen) * 0.5
    losses = []
    for _ in range(10):
        rng, tg = np.random.default_rng(0), torch.Generator().manual_seed(0)          # the same noise every step: a fixed objective
        losses.append(float(tr.train_step(x, y, np_rng=rng, generator=tg)))
    print(f"fine-tuning at 576 tokens: loss {losses[0]:.4f} -> {losses[-1]:.4f} (bound: below 0.8 x the first)")
    assert all(np.isfinite(losses)) and losses[-1] < 0.8 * losses[0], losses
    ema = tr.ema_state_dict()
    tr2 = Trainer(cfg, tc, device=_dev(), init_seed=9, max_batch=4)
    tr2.load_checkpoint(tr.checkpoint())
    assert tr2.global_step == tr.global_step
    for k, v in tr2.state_dict().items():
        assert torch.equal(v.cpu(), ema[k].cpu()), k
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict(ema)
    sig = torch.tensor([[0.3], [0.8]])
    out = m(x[:2].to(_dev()), sig.to(_dev()), y[:2].to(_dev())).float().cpu().numpy()
    ref = TorchRefDenoiser(asdict(cfg), {k: v.cpu().numpy() for k, v in ema.items()})(x[:2], sig, y[:2]).numpy()
    r = rel_rms(out, ref)
    print(f"fine-tuned EMA weights, inference forward vs restatement: rel-rms {r:.2e} (bound {FWD_TOL})")
    assert out.shape == (2, 4, 48, 48) and r <= FWD_TOL


def test_training_grid_domain_edges():
    """G = 10 (not a multiple of 4) and G = 66 (past 64) are refused with a message that names the rule; G = 64 (4096 tokens) builds."""
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    for S in (20, 132):
        with pytest.raises(RuntimeError, match=r"multiple of 4, 4 <= G <= 64"):
            Trainer(DenoiserConfig(image_size=S, n_channels=4, n_layers=1), device=_dev(), init_seed=1, max_batch=1)
    cfg = DenoiserConfig(image_size=128, n_channels=4, n_layers=1)
    cfg_d = cfg.embed_dim
    tr = Trainer(cfg, device=_dev(), init_seed=1, max_batch=1)
    assert int(np.prod(tr.layout["denoiser_trans_block.pos_embed.weight"][1])) == 4096 * cfg_d

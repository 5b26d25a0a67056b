"""CPU: the float64 stage functions of tests/train_stage_refs.py against torch.autograd.

Chained from the inputs on a tiny model (2 blocks, one dropped label; an 8 x 8 grid, which the engine's whole-image depthwise kernels
take, and a 32 x 32 grid, which its banded ones take) the loss, the prediction and every parameter gradient equal autograd over
oracle.torch_ref.TorchRefDenoiser(dtype=float64).forward_graph to 1e-10 relative per tensor (float64 against float64; that restatement is
tied to the reference's own autograd by the g15 / g17 fixtures).  Each stage's backward is also held alone against autograd of its own
forward, so a pair of compensating mistakes in the chain cannot pass."""
import numpy as np
import pytest
import torch

import train_stage_refs as R

TOL = 1e-10


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _setup(image_size, seed):
    from transformer_latent_diffusion_amd import DenoiserConfig
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = DenoiserConfig(image_size=image_size, noise_embed_dims=32, patch_size=2, embed_dim=128, dropout=0, n_layers=2, text_emb_size=48, n_channels=4,
                         mlp_multiplier=2)
    sd = synth_state_dict(cfg, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    B = 3
    x = torch.randn(B, 4, image_size, image_size, generator=gen, dtype=torch.float64) * 0.8
    xn = x + torch.randn(B, 4, image_size, image_size, generator=gen, dtype=torch.float64) * 0.5
    lab = torch.randn(B, 48, generator=gen, dtype=torch.float64) * 0.5
    lab[1] = 0                                                                    # a dropped label
    nl = torch.tensor([0.07, 0.45, 0.9], dtype=torch.float64)
    return cfg, sd, xn, nl, lab, x


@pytest.mark.parametrize("image_size", [16, 64])
def test_chained_stages_equal_autograd_of_the_pinned_restatement(image_size):
    from oracle.torch_ref import TorchRefDenoiser
    cfg, sd, xn, nl, lab, x = _setup(image_size, 5)
    ref = TorchRefDenoiser(cfg, sd, dtype=torch.float64)
    params = {}
    for k, v in ref.w.items():
        if v.is_floating_point() and "angular_speeds" not in k:
            ref.w[k] = v.clone().requires_grad_(True)
            params[k] = ref.w[k]
    with torch.enable_grad():
        pred_ref = ref.forward_graph(xn, nl.view(-1, 1), lab)
        loss_ref = torch.nn.functional.mse_loss(pred_ref, x)
        grads_ref = dict(zip(params, torch.autograd.grad(loss_ref, list(params.values()))))
    w = {k: v.detach() for k, v in ref.w.items()}
    loss, pred, gr = R.chain(cfg, w, xn, nl, lab, x)
    assert abs(float(loss) - float(loss_ref.detach())) <= TOL * float(loss_ref.detach())
    assert _rel(pred, pred_ref.detach()) <= TOL
    assert set(gr) == set(grads_ref)
    worst = max((_rel(gr[k], grads_ref[k]), k) for k in gr)
    print(f"image {image_size}: worst gradient relative L2 {worst[0]:.2e} ({worst[1]})")
    for k in gr:
        assert gr[k].shape == grads_ref[k].shape, k
        assert _rel(gr[k], grads_ref[k]) <= TOL, (k, _rel(gr[k], grads_ref[k]))


def _vjp(fn, inputs, cot):
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    with torch.enable_grad():
        out = fn(*leaves)
        return torch.autograd.grad(out, leaves, cot)


def _rand(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64) * scale


def test_layernorm_backward_alone():
    gen = torch.Generator().manual_seed(1)
    x, g, b, dy = _rand(gen, 5, 7, 192) + 0.3, _rand(gen, 192), _rand(gen, 192), _rand(gen, 5, 7, 192)
    _, mean, rstd = R.ln_fwd(x, g, b)
    got = R.ln_bwd(dy, x, mean, rstd, g)
    want = _vjp(lambda x_, g_, b_: torch.nn.functional.layer_norm(x_, (192,), g_, b_, 1e-5), (x, g, b), dy)
    for a, r in zip(got, want):
        assert _rel(a, r) <= TOL


def test_gelu_and_linear_backward_alone():
    gen = torch.Generator().manual_seed(2)
    x, dy = _rand(gen, 4, 33, scale=2.0), _rand(gen, 4, 33)
    assert _rel(R.gelu(x), torch.nn.functional.gelu(x)) <= TOL
    assert _rel(dy * R.gelu_grad(x), _vjp(torch.nn.functional.gelu, (x,), dy)[0]) <= TOL
    W, b, dz = _rand(gen, 20, 33), _rand(gen, 20), _rand(gen, 4, 20)
    for a, r in zip(R.linear_bwd(dz, x, W), _vjp(torch.nn.functional.linear, (x, W, b), dz)):
        assert _rel(a, r) <= TOL


@pytest.mark.parametrize("N", [16, 144])
def test_attention_backward_alone(N):
    gen = torch.Generator().manual_seed(3)
    B, H, d = 2, 3, 192
    q, k, v, do = (_rand(gen, B, N, d) for _ in range(4))
    sp = lambda t: t.view(B, N, H, 64).transpose(1, 2)
    sdpa = lambda q_, k_, v_: torch.nn.functional.scaled_dot_product_attention(sp(q_), sp(k_), sp(v_)).transpose(1, 2).reshape(B, N, d)
    assert _rel(R.attn_fwd(q, k, v, H), sdpa(q, k, v)) <= TOL
    for a, r in zip(R.attn_bwd(q, k, v, do, H), _vjp(sdpa, (q, k, v), do)):
        assert _rel(a, r) <= TOL


@pytest.mark.parametrize("N", [48, 144])
@pytest.mark.parametrize("g_is_bf16", [False, True])
def test_attention_backward_rounding_model(N, g_is_bf16):
    """attn_bwd_model, the yardstick of the attention-backward class tests: with every rounding off it is attn_bwd (itself held against
    autograd here and in test_attention_backward_alone); with them on it differs from the exact result by a relative rms of the order of one
    bf16 rounding -- above 2^-10 (the final rounding alone gives 2^-9 / sqrt(3) = 1.1e-3) and below 2^-6 -- in dq, dk and dv."""
    gen = torch.Generator().manual_seed(8 + N)
    B, H, d = 2, 3, 192
    bf = R.bf16_round
    q, k, v = bf(_rand(gen, B, N, d, scale=1.5)), bf(_rand(gen, B, N, d)), bf(_rand(gen, B, N, d))
    g = _rand(gen, B, N, d, scale=0.1).float().double()
    if g_is_bf16:
        g = bf(g)
    o = R.attn_fwd(q, k, v, H)
    exact = R.attn_bwd(q, k, v, g, H)
    sp = lambda t: t.view(B, N, H, 64).transpose(1, 2)
    sdpa = lambda q_, k_, v_: torch.nn.functional.scaled_dot_product_attention(sp(q_), sp(k_), sp(v_)).transpose(1, 2).reshape(B, N, d)
    for a, r in zip(exact, _vjp(sdpa, (q, k, v), g)):
        assert _rel(a, r) <= TOL
    for a, r in zip(R.attn_bwd_model(q, k, v, o, g, H, g_is_bf16, rounded=False), exact):
        assert _rel(a, r) <= TOL
    model = R.attn_bwd_model(q, k, v, bf(o), g, H, g_is_bf16)
    for name, a, r in zip(("dq", "dk", "dv"), model, exact):
        e = _rel(a, r)
        print(f"N = {N}, bf16 g {g_is_bf16}: model vs exact {name} {e:.2e}")
        assert torch.equal(a, bf(a)) and 2.0 ** -10 < e < 2.0 ** -6, (name, e)
    if not g_is_bf16:           # the two forms differ only in delta: the fp32-g form keeps dO unrounded there
        other = R.attn_bwd_model(q, k, v, bf(o), g, H, True)
        assert not torch.equal(other[0], model[0]) and torch.equal(other[2], model[2])


def test_cross_attention_alone():
    gen = torch.Generator().manual_seed(4)
    B, N, H, d = 3, 20, 2, 128
    qc, kv, g = _rand(gen, B, N, d), _rand(gen, B, 2, 2 * d), _rand(gen, B, N, d)
    sp = lambda t: t.view(B, t.shape[1], H, 64).transpose(1, 2)

    def fwd(q_, kv_):
        k_, v_ = kv_.chunk(2, dim=2)
        return torch.nn.functional.scaled_dot_product_attention(sp(q_), sp(k_), sp(v_)).transpose(1, 2).reshape(B, N, d)
    out, p0 = R.cross_fwd(qc, kv, H)
    assert _rel(out, fwd(qc, kv)) <= TOL
    assert float(p0.min()) > 0 and float(p0.max()) < 1 and p0.shape == (B, N, H)
    # the engine's own form of the output: p0 v0 + (1 - p0) v1 per head
    v0, v1 = kv[:, 0, d:].view(B, 1, H, 64), kv[:, 1, d:].view(B, 1, H, 64)
    assert _rel((p0[..., None] * v0 + (1 - p0[..., None]) * v1).reshape(B, N, d), out) <= TOL
    for a, r in zip(R.cross_bwd(g, qc, kv, H), _vjp(fwd, (qc, kv), g)):
        assert _rel(a, r) <= TOL


@pytest.mark.parametrize("G", [4, 12])
def test_depthwise_convolution_alone(G):
    gen = torch.Generator().manual_seed(6)
    B, Cc = 2, 10
    h, w, b, dhc = _rand(gen, B, G * G, Cc), _rand(gen, Cc, 9), _rand(gen, Cc), _rand(gen, B, G * G, Cc)

    def fwd(h_, w_, b_):
        t = h_.transpose(1, 2).reshape(B, Cc, G, G)
        t = torch.nn.functional.conv2d(t, w_.view(Cc, 1, 3, 3), b_, padding=1, groups=Cc)
        return t.reshape(B, Cc, G * G).transpose(1, 2)
    assert _rel(R.dwconv_fwd(h, w, b, G), fwd(h, w, b)) <= TOL
    for a, r in zip(R.dwconv_bwd(dhc, h, w, G), _vjp(fwd, (h, w, b), dhc)):
        assert _rel(a, r) <= TOL


def test_patches_and_loss_alone():
    gen = torch.Generator().manual_seed(7)
    x = _rand(gen, 2, 3, 8, 8)
    cw, cb = _rand(gen, 12, 3, 2, 2), _rand(gen, 12)
    conv = torch.nn.functional.conv2d(x, cw, cb, stride=2).reshape(2, 12, 16).transpose(1, 2)
    assert _rel(R.linear_fwd(R.patchify(x, 2), cw.reshape(12, -1), cb), conv) <= TOL
    assert torch.equal(R.unpatchify(R.patchify(x, 2), 3, 2), x)
    out, tgt = _rand(gen, 2, 16, 12), _rand(gen, 2, 3, 8, 8)
    loss, dout, row = R.mse_fwd(out, R.patchify(tgt, 2))
    fn = lambda o: torch.nn.functional.mse_loss(R.unpatchify(o, 3, 2), tgt)
    assert abs(float(loss) - float(fn(out))) <= TOL * float(loss)
    assert _rel(dout, _vjp(fn, (out,), torch.ones((), dtype=torch.float64))[0]) <= TOL
    assert abs(float(row.sum()) / out.numel() - float(loss)) <= TOL * float(loss)
    nl, ang = torch.tensor([0.1, 0.7], dtype=torch.float64), _rand(gen, 5).abs() * 10
    a = nl.view(-1, 1) * ang
    assert torch.equal(R.sinusoid(nl, ang), torch.cat([a.sin(), a.cos()], -1))

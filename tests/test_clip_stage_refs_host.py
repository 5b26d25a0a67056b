"""CPU: the float64 stage functions of the CLIP text tower (tests/clip_stage_refs.py), chained from the tokens, against
oracle/clip_ref.py (the fp32 restatement of CLIP.encode_text) and against the fixture captured from transformers'
CLIPTextModelWithProjection (g13, both geometries) -- ``text_embeds`` and ``last_hidden_state``, at the 1e-5 rel-rms / 1e-4 max-abs
of tests/test_clip_host.py.  The GPU stage test compares the engine with these functions, so they are held here first."""
import numpy as np
import pytest
import torch

import clip_stage_refs as R
from oracle.clip_ref import TorchRefClipText
from test_clip_host import TINY, _tokens, load_g13
from transformer_latent_diffusion_amd.clip_text import synth_clip_state_dict

FP32_REF_TOL = 1e-5       # test_clip_host.test_restatement_pinned_against_transformers_clip


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(np.mean(b ** 2)))


def _w(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("tag", ["tiny", "l14"])
def test_chain_against_the_transformers_fixture(tag):
    cfg, sd, text, want, want_hid = load_g13(tag)
    got, hid = R.chain(cfg, _w(sd), text, return_hidden=True)
    assert got.dtype == torch.float64 and got.shape == want.shape
    e, eh, ea = _rel(got.numpy(), want), _rel(hid.numpy()[:2], want_hid), float(np.abs(got.numpy() - want).max())
    print(f"{tag}: text_embeds rel-rms {e:.2e} max-abs {ea:.2e}, last_hidden_state rel-rms {eh:.2e}")
    assert e < FP32_REF_TOL and ea < 1e-4 and eh < FP32_REF_TOL


def test_chain_against_the_oracle():
    sd = synth_clip_state_dict(TINY, 3)
    text = _tokens(TINY, 11, 1)
    want, want_hid = TorchRefClipText(TINY, sd).encode_text(text, return_hidden=True)
    got, hid = R.chain(TINY, _w(sd), text, return_hidden=True)
    assert _rel(got.numpy(), want.numpy()) < FP32_REF_TOL and _rel(hid.numpy(), want_hid.numpy()) < FP32_REF_TOL


def test_stage_functions_one_by_one():
    """Each function against an independent torch statement in float64 (1e-12: both float64)."""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(5)
    B, ctx, W = 3, 7, 128
    x, add = torch.randn(B * ctx, W, generator=g, dtype=torch.float64), torch.randn(B * ctx, W, generator=g, dtype=torch.float64)
    bias, gamma, beta = (torch.randn(W, generator=g, dtype=torch.float64) for _ in range(3))
    s, h = R.add_layer_norm(x, add, bias, gamma, beta)
    assert torch.equal(s, x + add + bias) and torch.allclose(h, F.layer_norm(x + add + bias, (W,), gamma, beta, 1e-5), atol=1e-12)
    s0, h0 = R.add_layer_norm(x, None, None, gamma, beta)
    assert torch.equal(s0, x) and torch.allclose(h0, F.layer_norm(x, (W,), gamma, beta, 1e-5), atol=1e-12)
    mha = torch.nn.MultiheadAttention(W, W // 64, batch_first=True, dtype=torch.float64).eval()
    with torch.no_grad():
        qkv = R.in_proj(x, mha.in_proj_weight, mha.in_proj_bias)
        att = R.causal_attention(qkv, B, ctx)
        mine = R.out_proj(att, mha.out_proj.weight) + mha.out_proj.bias
        mask = torch.full((ctx, ctx), float("-inf"), dtype=torch.float64).triu_(1)
        xs = x.view(B, ctx, W)
        want = mha(xs, xs, xs, need_weights=False, attn_mask=mask)[0].reshape(B * ctx, W)
    assert torch.allclose(mine, want, atol=1e-12)
    assert torch.allclose(R.quick_gelu(x), x * torch.sigmoid(1.702 * x), atol=0)
    eot = torch.tensor([0, 6, 3])
    pooled = R.final_add_layer_norm(x, add, bias, eot, gamma, beta, ctx)
    assert torch.allclose(pooled, h.view(B, ctx, W)[torch.arange(B), eot], atol=1e-12)
    proj = torch.randn(W, 32, generator=g, dtype=torch.float64)
    assert torch.allclose(R.projection(pooled, proj.t().contiguous()), pooled @ proj, atol=1e-12)
    tok = torch.randint(0, 50, (B, ctx), generator=g)
    emb, pos = torch.randn(50, W, generator=g), torch.randn(ctx, W, generator=g)
    assert torch.equal(R.embed(tok, emb, pos), (emb.double()[tok] + pos.double()).reshape(B * ctx, W))

"""Float64 statements of every transition of the CLIP image tower (csrc/tld_clip_vision.hip), one plain torch function each.

Restated from openai/CLIP clip/model.py (VisionTransformer.forward, ResidualAttentionBlock without a mask, QuickGELU, LayerNorm).  The stages
the image tower shares with the text tower (LayerNorm, the projections, QuickGELU, the residual add, the fp32 projection) are the functions of
tests/clip_stage_refs.py; what is stated here is the patch embedding (im2col + GEMM), the class token / positional table / ln_pre row kernel,
the unmasked attention -- exactly (``attention_exact``) and with the roundings clip_vis_attn_kernel documents (``attention_model``) -- and the
class-token pooling.  tests/test_clip_vision_host.py chains them and holds the chain against transformers' CLIPVisionModelWithProjection.

Rows are [T, W] with T = batch * n, n = g * g + 1 (sample major, class token first), the engine's layout.
"""
import math

import torch

import clip_stage_refs as R
from clip_stage_refs import HEAD_DIM, _d


def bf16(t):
    """Round to bf16 (RNE) and return float64: a value as a bf16 buffer of the engine holds it."""
    return t.to(torch.float32).to(torch.bfloat16).double()


def padded_k(patch):
    """Kp: the contraction 3 p*p rounded up to the multiple of 64 the GEMM takes."""
    return (3 * patch * patch + 63) // 64 * 64


def patches(pixels, patch):
    """im2col of conv1 (kernel = stride = patch): [B * g * g, Kp], row (b, gy, gx), column (c * p + py) * p + px, zero beyond 3 p*p."""
    x = _d(pixels)
    b, c, r, _ = x.shape
    g = r // patch
    rows = x.reshape(b, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(b * g * g, c * patch * patch)
    out = torch.zeros(b * g * g, padded_k(patch), dtype=torch.float64, device=x.device)
    out[:, :rows.shape[1]] = rows
    return out


def pack_conv_weight(conv_w, patch):
    """conv1.weight [W, 3, p, p] as the engine holds it: [W, Kp], zero beyond 3 p*p."""
    w = _d(conv_w).reshape(conv_w.shape[0], -1)
    out = torch.zeros(w.shape[0], padded_k(patch), dtype=torch.float64, device=w.device)
    out[:, :w.shape[1]] = w
    return out


def patch_embed(patch_rows, conv_w_packed):
    return R.linear(patch_rows, conv_w_packed)


def embed_ln_pre(emb, cls, pos, gamma, beta, batch):
    """clip_vis_embed_ln_kernel: ln_pre(cat(class_embedding, emb) + positional_embedding), [batch * n, W]."""
    emb = _d(emb)
    w = emb.shape[1]
    x = torch.cat([_d(cls).expand(batch, 1, w), emb.reshape(batch, -1, w)], dim=1) + _d(pos)
    return R.layer_norm(x, gamma, beta).reshape(-1, w)


def _split(qkv, batch, n):
    qkv = _d(qkv)
    w = qkv.shape[1] // 3
    heads = w // HEAD_DIM
    sp = lambda t: t.reshape(batch, n, heads, HEAD_DIM).transpose(1, 2)
    return [sp(qkv[:, i * w:(i + 1) * w]) for i in range(3)], w


def attention_exact(qkv, batch, n):
    """nn.MultiheadAttention without a mask on the packed in_proj rows [T, 3 W]: softmax(q k^T / 8) v per (sample, head).  Returns [T, W]."""
    (q, k, v), w = _split(qkv, batch, n)
    s = q @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
    return (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(batch * n, w)


def attention_model(qkv, batch, n):
    """The same with clip_vis_attn_kernel's documented roundings: q, k, v as stored (the caller passes the bf16 values); scores, the maximum,
    e = exp(s - max) and l = sum e exact (fp32 in the kernel: not modelled); e rounded to bf16 for the P V product; o = (bf16(e) v) / l rounded to
    bf16 on the store."""
    (q, k, v), w = _split(qkv, batch, n)
    s = q @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
    e = torch.exp(s - s.amax(dim=-1, keepdim=True))
    o = (bf16(e) @ v) / e.sum(dim=-1, keepdim=True)
    return bf16(o.transpose(1, 2).reshape(batch * n, w))


def class_add_layer_norm(x, add, bias, gamma, beta, n):
    """clip_final_ln_kernel with no EOT table: the last block's residual add and ln_post on row 0 of each sample: [B, W]."""
    batch = x.shape[0] // n
    zero = torch.zeros(batch, dtype=torch.long, device=x.device)
    return R.final_add_layer_norm(x, add, bias, zero, gamma, beta, n)


def chain(cfg, w, pixels, rounded=False):
    """The whole tower from these functions; w is an openai/CLIP-keyed state_dict of tensors, pixels [B, 3, R, R].  Returns image_embeds [B, E].
    rounded: the rounding model of the engine -- bf16 GEMM operands (weights and the stages the engine stores as bf16: patches, h1, h2, qkv,
    f_pre, f) and attention_model in place of attention_exact; everything else stays float64."""
    rd = bf16 if rounded else _d
    att_fn = attention_model if rounded else attention_exact
    b, p, n = pixels.shape[0], cfg.patch_size, cfg.tokens
    v = lambda k: w["visual." + k]
    blk = lambda i, k: w[f"visual.transformer.resblocks.{i}.{k}"]
    emb = patch_embed(rd(patches(pixels, p)), rd(pack_conv_weight(v("conv1.weight"), p)))
    x = embed_ln_pre(emb, v("class_embedding"), v("positional_embedding"), v("ln_pre.weight"), v("ln_pre.bias"), b)
    x, h = R.add_layer_norm(x, None, None, blk(0, "ln_1.weight"), blk(0, "ln_1.bias"))
    for i in range(cfg.layers):
        qkv = rd(R.in_proj(rd(h), rd(blk(i, "attn.in_proj_weight")), blk(i, "attn.in_proj_bias")))
        att = att_fn(qkv, b, n)
        x, h = R.add_layer_norm(x, R.out_proj(att, rd(blk(i, "attn.out_proj.weight"))), blk(i, "attn.out_proj.bias"), blk(i, "ln_2.weight"), blk(i, "ln_2.bias"))
        f = rd(R.quick_gelu(rd(R.c_fc(rd(h), rd(blk(i, "mlp.c_fc.weight")), blk(i, "mlp.c_fc.bias")))))
        mlp = R.c_proj(f, rd(blk(i, "mlp.c_proj.weight")))
        if i + 1 < cfg.layers:
            x, h = R.add_layer_norm(x, mlp, blk(i, "mlp.c_proj.bias"), blk(i + 1, "ln_1.weight"), blk(i + 1, "ln_1.bias"))
    pooled = class_add_layer_norm(x, mlp, blk(cfg.layers - 1, "mlp.c_proj.bias"), v("ln_post.weight"), v("ln_post.bias"), n)
    return R.projection(pooled, _d(v("proj")).t())

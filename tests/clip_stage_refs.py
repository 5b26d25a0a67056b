"""Float64 statements of every transition of the CLIP text tower (csrc/tld_clip.hip), one plain torch function each.

Restated from openai/CLIP clip/model.py (CLIP.encode_text, ResidualAttentionBlock, QuickGELU, LayerNorm), as oracle/clip_ref.py does for
the whole tower; here each function takes its stage inputs and operands as arguments, so the GPU stage test (tests/test_gpu_clip_stages.py)
can feed it the engine's own snapshot of the inputs and the engine's own operands.  Every function works on any device and converts to
float64 itself.  tests/test_clip_stage_refs_host.py chains them from the tokens and holds the chain against oracle/clip_ref.py and the
transformers fixture g13.

Rows are [T, W] with T = batch * ctx (sample major), the engine's layout.
"""
import math

import torch

LN_EPS = 1e-5             # kLnEps (csrc/tld_common.h); nn.LayerNorm's default
QUICKGELU_ALPHA = 1.702   # clip/model.py QuickGELU; clip_quickgelu_kernel
HEAD_DIM = 64             # tld_clip_create: head_dim must be 64


def _d(t):
    return t.double()


def embed(tokens, tok_emb, pos):
    """x0[b * ctx + i] = token_embedding[tokens[b, i]] + positional_embedding[i]        (clip_embed_kernel; ids as given: no clamp here)"""
    b, n = tokens.shape
    return (_d(tok_emb)[tokens.long()] + _d(pos)[:n]).reshape(b * n, -1)


def layer_norm(x, gamma, beta):
    x = _d(x)
    mean = x.mean(dim=-1, keepdim=True)
    var = (x - mean).pow(2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + LN_EPS) * _d(gamma) + _d(beta)


def add_layer_norm(x, add, bias, gamma, beta):
    """clip_add_ln_kernel: (x + add + bias, LayerNorm of that); add is None at the tower's entry (LayerNorm only)."""
    x = _d(x) if add is None else _d(x) + _d(add) + _d(bias)
    return x, layer_norm(x, gamma, beta)


def linear(a, w, bias=None):
    """a [T, K] times w [N, K] transposed, plus bias: in_proj, out_proj, c_fc, c_proj (the fp32 GEMM outputs carry no bias: bias=None)."""
    y = _d(a) @ _d(w).t()
    return y if bias is None else y + _d(bias)


def in_proj(h1, w, bias):
    return linear(h1, w, bias)


def out_proj(att, w):
    return linear(att, w)


def c_fc(h2, w, bias):
    return linear(h2, w, bias)


def c_proj(f, w):
    return linear(f, w)


def causal_attention(qkv, batch, ctx):
    """nn.MultiheadAttention with the mask of build_attention_mask on the packed in_proj rows [T, 3 W] (q | k | v, head h at columns h * 64):
    s_ij = q_i . k_j / sqrt(64) for j <= i, softmax over j, o_i = sum_j p_ij v_j.  Returns [T, W]."""
    qkv = _d(qkv)
    w = qkv.shape[1] // 3
    heads = w // HEAD_DIM
    sp = lambda t: t.reshape(batch, ctx, heads, HEAD_DIM).transpose(1, 2)
    q, k, v = (sp(qkv[:, i * w:(i + 1) * w]) for i in range(3))
    s = q @ k.transpose(-1, -2) / math.sqrt(HEAD_DIM)
    mask = torch.full((ctx, ctx), float("-inf"), dtype=torch.float64, device=qkv.device).triu_(1)
    return (torch.softmax(s + mask, dim=-1) @ v).transpose(1, 2).reshape(batch * ctx, w)


def quick_gelu(x):
    x = _d(x)
    return x * torch.sigmoid(QUICKGELU_ALPHA * x)


def final_add_layer_norm(x, add, bias, eot, gamma, beta, ctx):
    """clip_final_ln_kernel: the last block's residual add and ln_final on the row of each sample's EOT position only: [B, W]."""
    rows = torch.arange(eot.shape[0], device=eot.device) * ctx + eot.long()
    return layer_norm(_d(x)[rows] + _d(add)[rows] + _d(bias), gamma, beta)


def projection(pooled, proj_t):
    """pooled [B, W] @ text_projection, with the operand as the engine holds it: proj_t = text_projection^T [E, W]."""
    return _d(pooled) @ _d(proj_t).t()


def chain(cfg, w, tokens, return_hidden=False):
    """The whole tower from these functions: w is an openai/CLIP-keyed state_dict of tensors.  Returns text_embeds [B, E] and, on request,
    ln_final of every row [B, ctx, W] (transformers' last_hidden_state)."""
    b, n = tokens.shape
    blk = lambda i, k: w[f"transformer.resblocks.{i}.{k}"]
    x = embed(tokens, w["token_embedding.weight"], w["positional_embedding"])
    x, h = add_layer_norm(x, None, None, blk(0, "ln_1.weight"), blk(0, "ln_1.bias"))
    for i in range(cfg.layers):
        att = causal_attention(in_proj(h, blk(i, "attn.in_proj_weight"), blk(i, "attn.in_proj_bias")), b, n)
        x, h = add_layer_norm(x, out_proj(att, blk(i, "attn.out_proj.weight")), blk(i, "attn.out_proj.bias"), blk(i, "ln_2.weight"), blk(i, "ln_2.bias"))
        mlp = c_proj(quick_gelu(c_fc(h, blk(i, "mlp.c_fc.weight"), blk(i, "mlp.c_fc.bias"))), blk(i, "mlp.c_proj.weight"))
        if i + 1 < cfg.layers:
            x, h = add_layer_norm(x, mlp, blk(i, "mlp.c_proj.bias"), blk(i + 1, "ln_1.weight"), blk(i + 1, "ln_1.bias"))
    last = cfg.layers - 1
    eot = tokens.argmax(dim=-1)
    pooled = final_add_layer_norm(x, mlp, blk(last, "mlp.c_proj.bias"), eot, w["ln_final.weight"], w["ln_final.bias"], n)
    out = projection(pooled, _d(w["text_projection"]).t())
    if not return_hidden:
        return out
    hidden = layer_norm(x + mlp + _d(blk(last, "mlp.c_proj.bias")), w["ln_final.weight"], w["ln_final.bias"]).reshape(b, n, -1)
    return out, hidden

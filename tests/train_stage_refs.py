"""Float64 statements of every stage of the training step (forward and local vector-Jacobian products), one function per transition.

Test infrastructure: tests/test_gpu_train_stages.py feeds these with the engine's own snapshots (tld_train_set_debug) and compares their
output with the engine's next snapshot; tests/test_train_stage_refs_host.py chains them on the host and holds the chain, and every backward
on its own, against torch.autograd (over oracle/torch_ref.TorchRefDenoiser for the chain), so that a wrong reference cannot agree with a
wrong kernel.  They restate oracle/torch_ref.py (tld/denoiser.py, tld/transformer_blocks.py of the reference) with explicit backward
formulas; nothing here differentiates automatically.  Tensors are token-major [rows, features] / [B, N, features], any device, float64.
"""
import math

import torch

EPS = 1e-5
BLK = "denoiser_trans_block."


# ---- elementwise / rows ---------------------------------------------------------------------------------------------------------------
def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def ln_fwd(x, gamma, beta):
    """LayerNorm over the last axis (biased variance, eps 1e-5): (out, mean, rstd), mean / rstd shaped [..., 1]."""
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS)
    return (x - mean) * rstd * gamma + beta, mean, rstd


def ln_bwd(dy, x, mean, rstd, gamma):
    """(dx, dgamma, dbeta) of ln_fwd; the parameter gradients summed over every leading axis."""
    xh = (x - mean) * rstd
    g = dy * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    w = x.shape[-1]
    return dx, (dy * xh).reshape(-1, w).sum(0), dy.reshape(-1, w).sum(0)


def linear_fwd(x, W, b=None):
    out = x @ W.T
    return out if b is None else out + b


def linear_bwd(dy, x, W):
    """(dx, dW, db) of out = x W^T + b over rows."""
    dy2, x2 = dy.reshape(-1, dy.shape[-1]), x.reshape(-1, x.shape[-1])
    return dy @ W, dy2.T @ x2, dy2.sum(0)


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _heads(t, H):
    b, n, d = t.shape
    return t.view(b, n, H, d // H).transpose(1, 2)


def _merge(t):
    b, h, n, k = t.shape
    return t.transpose(1, 2).reshape(b, n, h * k)


def attn_fwd(q, k, v, H):
    """softmax(q k^T / sqrt(head_dim)) v per head; q, k, v [B, N, d]."""
    qh, kh, vh = _heads(q, H), _heads(k, H), _heads(v, H)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1]), dim=-1)
    return _merge(p @ vh)


def attn_bwd(q, k, v, do, H):
    qh, kh, vh, doh = _heads(q, H), _heads(k, H), _heads(v, H), _heads(do, H)
    sc = 1.0 / math.sqrt(qh.shape[-1])
    p = torch.softmax(qh @ kh.transpose(-1, -2) * sc, dim=-1)
    dv = p.transpose(-1, -2) @ doh
    dp = doh @ vh.transpose(-1, -2)
    ds = p * (dp - (dp * p).sum(-1, keepdim=True)) * sc
    return _merge(ds @ kh), _merge(ds.transpose(-1, -2) @ qh), _merge(dv)


def bf16_round(t):
    """The bf16 rounding of an fp32 value, as a float64 tensor (the kernels round fp32 accumulators)."""
    return t.float().bfloat16().to(t.dtype)


def attn_bwd_model(q, k, v, o, g, H, g_is_bf16, rounded=True):
    """Rounding model of csrc/tld_train_attn.hip: attn_bwd in float64 with the roundings the kernel documents and no others.  q, k, v, g
    [B, N, d]; o [B, N, d] is the forward's output as the kernel reads it (bf16).  dO is rounded to bf16 for the dP, dV and dK products;
    delta = dO . O takes dO unrounded when the kernel gets an fp32 gradient and the bf16 dO when it gets a bf16 one; P stays unrounded
    inside dS = P o (dP - delta); dS is rounded to bf16 before dS K and dS^T Q, P before P^T dO; each output is scaled (1/8 for dq and dk)
    and rounded once to bf16.  rounded=False switches every rounding off: attn_bwd again, with delta from o."""
    r = bf16_round if rounded else (lambda t: t)
    qh, kh, vh, oh, gh = (_heads(t, H) for t in (q, k, v, o, g))
    sc = 1.0 / math.sqrt(qh.shape[-1])
    gb = r(gh)
    p = torch.softmax(qh @ kh.transpose(-1, -2) * sc, dim=-1)
    delta = ((gb if g_is_bf16 else gh) * oh).sum(-1, keepdim=True)
    ds = r(p * (gb @ vh.transpose(-1, -2) - delta))
    dv = r(p).transpose(-1, -2) @ gb
    return r(_merge(ds @ kh * sc)), r(_merge(ds.transpose(-1, -2) @ qh * sc)), r(_merge(dv))


def cross_fwd(qc, kv, H):
    """Attention of every token over the two conditioning tokens: qc [B, N, d], kv [B, 2, 2 d] = (k | v) -> (out [B, N, d], p0 [B, N, H])."""
    d = qc.shape[-1]
    k, v = kv[..., :d], kv[..., d:]
    qh, kh, vh = _heads(qc, H), _heads(k, H), _heads(v, H)
    p = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d // H), dim=-1)          # [B, H, N, 2]
    return _merge(p @ vh), p[..., 0].transpose(1, 2)


def cross_bwd(g, qc, kv, H):
    """(dqc [B, N, d], dkv [B, 2, 2 d]) of cross_fwd."""
    d = qc.shape[-1]
    k, v = kv[..., :d], kv[..., d:]
    dq, dk, dv = attn_bwd(qc, k, v, g, H)
    return dq, torch.cat([dk, dv], dim=-1)


# ---- depthwise 3 x 3 (zero padding, cross-correlation) on channels-last tokens --------------------------------------------------------------
def _img(t, G):
    return t.view(t.shape[0], G, G, t.shape[-1])


def dwconv_fwd(h, w, b, G):
    """h [B, N, C], w [C, 9] (ky, kx row-major), b [C]: out[y, x] = b + sum w[ky, kx] h[y + ky - 1, x + kx - 1]."""
    x = torch.nn.functional.pad(_img(h, G), (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(_img(h, G))
    for ky in range(3):
        for kx in range(3):
            out = out + w[:, ky * 3 + kx] * x[:, ky:ky + G, kx:kx + G]
    if b is not None:
        out = out + b
    return out.reshape(h.shape)


def dwconv_bwd(dhc, h, w, G):
    """(dh, dw [C, 9], db [C]) of dwconv_fwd."""
    dp = torch.nn.functional.pad(_img(dhc, G), (0, 0, 1, 1, 1, 1))
    hp = torch.nn.functional.pad(_img(h, G), (0, 0, 1, 1, 1, 1))
    dh = torch.zeros_like(_img(h, G))
    dw = []
    for ky in range(3):
        for kx in range(3):
            dh = dh + w[:, ky * 3 + kx] * dp[:, 2 - ky:2 - ky + G, 2 - kx:2 - kx + G]
            dw.append((_img(dhc, G) * hp[:, ky:ky + G, kx:kx + G]).sum((0, 1, 2)))
    return dh.reshape(h.shape), torch.stack(dw, dim=1), dhc.reshape(-1, dhc.shape[-1]).sum(0)


# ---- ends -----------------------------------------------------------------------------------------------------------------------------
def patchify(x, patch):
    """[B, C, S, S] -> [B, N, C p p] with features ordered (c, p1, p2): the operand of the patch convolution and the unpatchify inverse."""
    b, c, s, _ = x.shape
    g = s // patch
    return x.view(b, c, g, patch, g, patch).permute(0, 2, 4, 1, 3, 5).reshape(b, g * g, c * patch * patch)


def unpatchify(o, C, patch):
    b, n, _ = o.shape
    g = int(math.isqrt(n))
    return o.view(b, g, g, C, patch, patch).permute(0, 3, 1, 4, 2, 5).reshape(b, C, g * patch, g * patch)


def sinusoid(noise_level, angular):
    a = noise_level.view(-1, 1) * angular
    return torch.cat([torch.sin(a), torch.cos(a)], dim=-1)


def mse_fwd(out, target_tok):
    """out, target_tok [B, N, pd] -> (loss, dout = d loss / d out, row_loss = squared error per token)."""
    diff = out - target_tok
    return (diff ** 2).mean(), 2.0 * diff / diff.numel(), (diff ** 2).sum(-1)


# ---- the chain (host check against autograd) ----------------------------------------------------------------------------------------------
def chain(cfg, w, x_noisy, noise_level, label, target):
    """Every stage above in order: (loss, pred, {key: grad}) for a reference-keyed float64 state dict `w`."""
    c = cfg if isinstance(cfg, dict) else cfg.__dict__
    d, L, patch, C = c["embed_dim"], c["n_layers"], c["patch_size"], c["n_channels"]
    H, G = d // 64, c["image_size"] // patch
    N = G * G
    gr = {}
    pe = BLK + "patchify_and_embed."
    # forward
    sinb = sinusoid(noise_level, w["fourier_feats.0.angular_speeds"])
    h1 = linear_fwd(sinb, w["fourier_feats.1.weight"], w["fourier_feats.1.bias"])
    g1 = gelu(h1)
    nz = linear_fwd(g1, w["fourier_feats.3.weight"], w["fourier_feats.3.bias"])
    lb = linear_fwd(label, w["label_proj.weight"], w["label_proj.bias"])
    ycat = torch.stack([nz, lb], dim=1)
    y, ym, yr = ln_fwd(ycat, w["norm.weight"], w["norm.bias"])
    pt = patchify(x_noisy, patch)
    pd = pt.shape[-1]
    p16 = linear_fwd(pt, w[pe + "0.weight"].reshape(pd, -1), w[pe + "0.bias"])
    p16n, m1, r1 = ln_fwd(p16, w[pe + "2.weight"], w[pe + "2.bias"])
    e = linear_fwd(p16n, w[pe + "3.weight"], w[pe + "3.bias"])
    en, m2, r2 = ln_fwd(e, w[pe + "4.weight"], w[pe + "4.bias"])
    x = en + w[BLK + "pos_embed.weight"][:N]
    sv = []
    for i in range(L):
        p = f"{BLK}decoder_blocks.{i}."
        s = {"x1": x}
        s["a1"], s["m1"], s["r1"] = ln_fwd(x, w[p + "norm1.weight"], w[p + "norm1.bias"])
        s["q"], s["k"], s["v"] = linear_fwd(s["a1"], w[p + "self_attention.qkv_linear.weight"]).chunk(3, dim=-1)
        s["x2"] = x + attn_fwd(s["q"], s["k"], s["v"], H)
        s["a2"], s["m2"], s["r2"] = ln_fwd(s["x2"], w[p + "norm2.weight"], w[p + "norm2.bias"])
        s["qc"] = linear_fwd(s["a2"], w[p + "cross_attention.q_linear.weight"])
        s["kv"] = linear_fwd(y, w[p + "cross_attention.kv_linear.weight"])
        cr, _ = cross_fwd(s["qc"], s["kv"], H)
        s["x3"] = s["x2"] + cr
        s["a3"], s["m3"], s["r3"] = ln_fwd(s["x3"], w[p + "norm3.weight"], w[p + "norm3.bias"])
        s["h"] = linear_fwd(s["a3"], w[p + "mlp.mlp.0.weight"].reshape(-1, d), w[p + "mlp.mlp.0.bias"])
        s["hc"] = dwconv_fwd(s["h"], w[p + "mlp.mlp.1.weight"].reshape(-1, 9), w[p + "mlp.mlp.1.bias"], G)
        s["gl"] = gelu(s["hc"])
        x = s["x3"] + linear_fwd(s["gl"], w[p + "mlp.mlp.3.weight"].reshape(d, -1), w[p + "mlp.mlp.3.bias"])
        sv.append(s)
    out = linear_fwd(x, w[BLK + "out_proj.0.weight"], w[BLK + "out_proj.0.bias"])
    loss, dout, _ = mse_fwd(out, patchify(target, patch))
    pred = unpatchify(out, C, patch)
    # backward
    gx, gr[BLK + "out_proj.0.weight"], gr[BLK + "out_proj.0.bias"] = linear_bwd(dout, x, w[BLK + "out_proj.0.weight"])
    dy = torch.zeros_like(y)
    for i in reversed(range(L)):
        p = f"{BLK}decoder_blocks.{i}."
        s = sv[i]
        dg, dW, gr[p + "mlp.mlp.3.bias"] = linear_bwd(gx, s["gl"], w[p + "mlp.mlp.3.weight"].reshape(d, -1))
        gr[p + "mlp.mlp.3.weight"] = dW.reshape(w[p + "mlp.mlp.3.weight"].shape)
        dhc = dg * gelu_grad(s["hc"])
        dh, dw, gr[p + "mlp.mlp.1.bias"] = dwconv_bwd(dhc, s["h"], w[p + "mlp.mlp.1.weight"].reshape(-1, 9), G)
        gr[p + "mlp.mlp.1.weight"] = dw.reshape(w[p + "mlp.mlp.1.weight"].shape)
        da3, dW, gr[p + "mlp.mlp.0.bias"] = linear_bwd(dh, s["a3"], w[p + "mlp.mlp.0.weight"].reshape(-1, d))
        gr[p + "mlp.mlp.0.weight"] = dW.reshape(w[p + "mlp.mlp.0.weight"].shape)
        dx, gr[p + "norm3.weight"], gr[p + "norm3.bias"] = ln_bwd(da3, s["x3"], s["m3"], s["r3"], w[p + "norm3.weight"])
        gx = gx + dx
        dqc, dkv = cross_bwd(gx, s["qc"], s["kv"], H)
        dyi, gr[p + "cross_attention.kv_linear.weight"], _ = linear_bwd(dkv, y, w[p + "cross_attention.kv_linear.weight"])
        dy = dy + dyi
        da2, gr[p + "cross_attention.q_linear.weight"], _ = linear_bwd(dqc, s["a2"], w[p + "cross_attention.q_linear.weight"])
        dx, gr[p + "norm2.weight"], gr[p + "norm2.bias"] = ln_bwd(da2, s["x2"], s["m2"], s["r2"], w[p + "norm2.weight"])
        gx = gx + dx
        dqkv = torch.cat(attn_bwd(s["q"], s["k"], s["v"], gx, H), dim=-1)
        da1, gr[p + "self_attention.qkv_linear.weight"], _ = linear_bwd(dqkv, s["a1"], w[p + "self_attention.qkv_linear.weight"])
        dx, gr[p + "norm1.weight"], gr[p + "norm1.bias"] = ln_bwd(da1, s["x1"], s["m1"], s["r1"], w[p + "norm1.weight"])
        gx = gx + dx
    full = torch.zeros_like(w[BLK + "pos_embed.weight"])
    full[:N] = gx.sum(0)
    gr[BLK + "pos_embed.weight"] = full
    de, gr[pe + "4.weight"], gr[pe + "4.bias"] = ln_bwd(gx, e, m2, r2, w[pe + "4.weight"])
    dpn, gr[pe + "3.weight"], gr[pe + "3.bias"] = linear_bwd(de, p16n, w[pe + "3.weight"])
    dp16, gr[pe + "2.weight"], gr[pe + "2.bias"] = ln_bwd(dpn, p16, m1, r1, w[pe + "2.weight"])
    _, dW, gr[pe + "0.bias"] = linear_bwd(dp16, pt, w[pe + "0.weight"].reshape(pd, -1))
    gr[pe + "0.weight"] = dW.reshape(w[pe + "0.weight"].shape)
    dycat, gr["norm.weight"], gr["norm.bias"] = ln_bwd(dy, ycat, ym, yr, w["norm.weight"])
    _, gr["label_proj.weight"], gr["label_proj.bias"] = linear_bwd(dycat[:, 1], label, w["label_proj.weight"])
    dg1, gr["fourier_feats.3.weight"], gr["fourier_feats.3.bias"] = linear_bwd(dycat[:, 0], g1, w["fourier_feats.3.weight"])
    dh1 = dg1 * gelu_grad(h1)
    _, gr["fourier_feats.1.weight"], gr["fourier_feats.1.bias"] = linear_bwd(dh1, sinb, w["fourier_feats.1.weight"])
    return loss, pred, gr

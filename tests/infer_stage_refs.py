"""Float64 statements of every transition of the inference forward and of the sampler's elementwise steps, one function per transition.

Test infrastructure: tests/test_gpu_forward_stages.py feeds these with the engine's own snapshots (tld_engine_set_debug) and operands and compares
their output with the engine's next snapshot; tests/test_infer_stage_refs_host.py chains them on the host and holds the chain against the stage
arrays of the reference fixtures (g1, g5) and the update functions against the sampler traces (g2), so that a wrong reference cannot agree with a
wrong kernel.  Operations the training step shares (LayerNorm, attention, cross-attention, depthwise conv, patchify ...) come from
tests/train_stage_refs.py.  Tensors are token-major [rows, features] / [B, N, features], any device, float64.

Two kinds of function live here: the exact statement of a transition, and -- for the kernels that round inside (`*_model`) -- the same statement
with the intermediate roundings the kernels document applied (DESIGN.md 7.6 lists them with the kernel lines).  The relative rms between the two
is the yardstick of the MODELLED tolerance class.
"""
import math

import torch

import train_stage_refs as R
from train_stage_refs import BLK, EPS  # noqa: F401


def bf16(x):
    """Round to nearest-even bf16, returned in the input's type."""
    return x.float().bfloat16().to(x.dtype)


# ---- conditioning ---------------------------------------------------------------------------------------------------------------------------
def cond_sin(w, sigma):
    return R.sinusoid(sigma.reshape(-1), w["fourier_feats.0.angular_speeds"])


def cond_h1(w, sinb):
    return R.gelu(R.linear_fwd(sinb, w["fourier_feats.1.weight"], w["fourier_feats.1.bias"]))


def cond_noise_pre(w, h1):
    return R.linear_fwd(h1, w["fourier_feats.3.weight"], w["fourier_feats.3.bias"])


def cond_label_pre(w, label):
    return R.linear_fwd(label, w["label_proj.weight"], w["label_proj.bias"])


def cond_pre(w, sigma, label):
    """Pre-LayerNorm conditioning rows: (noise rows [Tn, d], label rows [Tl, d]) -- tld/denoiser.py:105-119."""
    return cond_noise_pre(w, cond_h1(w, cond_sin(w, sigma))), cond_label_pre(w, label)


def cond_y(w, pre):
    return R.ln_fwd(pre, w["norm.weight"], w["norm.bias"])[0]


def cond_tables(w, y, i, H):
    """Per-layer tables of token rows y [T, d]: kv [T, 2 d] = y Wkv^T, the folded query vectors wq [T, H, d] = gamma2 (Wq_h^T k_h / 8) and
    bwq [T, H] = beta2 . (Wq_h^T k_h / 8): the logit of a LayerNorm-2 row xhat against token t's head h is xhat . wq[t, h] / rstd-free + bwq[t, h]."""
    p = f"{BLK}decoder_blocks.{i}."
    d = y.shape[-1]
    kv = R.linear_fwd(y, w[p + "cross_attention.kv_linear.weight"])
    k = kv[:, :d].reshape(-1, H, d // H)
    Wq = w[p + "cross_attention.q_linear.weight"].reshape(H, d // H, d)
    raw = torch.einsum("thc,hcj->thj", k, Wq) / math.sqrt(d // H)
    return kv, raw * w[p + "norm2.weight"], (raw * w[p + "norm2.bias"]).sum(-1)


# ---- ends -------------------------------------------------------------------------------------------------------------------------------------
def embed(w, x, patch):
    """[B, C, S, S] -> tokens [B, N, d] before the store into the residual stream."""
    pe = BLK + "patchify_and_embed."
    pt = R.patchify(x, patch)
    pd = pt.shape[-1]
    p16 = R.linear_fwd(pt, w[pe + "0.weight"].reshape(pd, -1), w[pe + "0.bias"])
    p16n = R.ln_fwd(p16, w[pe + "2.weight"], w[pe + "2.bias"])[0]
    e = R.linear_fwd(p16n, w[pe + "3.weight"], w[pe + "3.bias"])
    en = R.ln_fwd(e, w[pe + "4.weight"], w[pe + "4.bias"])[0]
    return en + w[BLK + "pos_embed.weight"][:pt.shape[1]]


def tail(w, x, C, patch):
    """tokens [B, N, d] -> [B, C, S, S]."""
    return R.unpatchify(R.linear_fwd(x, w[BLK + "out_proj.0.weight"], w[BLK + "out_proj.0.bias"]), C, patch)


# ---- LayerNorm through statistics (the folds) --------------------------------------------------------------------------------------------------
def partial_sums(x, slots, first_block):
    """(sum, sum of squares) of the stored rows x [M, d] as the LayerNorm-1 fold reads them: [M, slots, 2].  Block 0 (written by the embedding
    kernel): the whole row in slot 0, zeros in slot 1.  Later blocks (written by the down projection / the split-K finisher): one slot per 96 columns."""
    M, d = x.shape
    if first_block:
        z = torch.zeros(M, 2, 2, dtype=x.dtype, device=x.device)
        z[:, 0, 0], z[:, 0, 1] = x.sum(-1), (x * x).sum(-1)
        return z
    g = x.view(M, slots, d // slots)
    return torch.stack([g.sum(-1), (g * g).sum(-1)], dim=-1)


def stats_from_sums(ps, d):
    """(mean, rstd) [M, 1] each from partial sums [M, n, 2]."""
    mean = ps[..., 0].sum(-1, keepdim=True) / d
    var = ps[..., 1].sum(-1, keepdim=True) / d - mean * mean
    return mean, 1.0 / torch.sqrt(var + EPS)


def row_stats(x):
    """(mean, rstd) [M, 2] of rows x."""
    _, m, r = R.ln_fwd(x, 1.0, 0.0)
    return torch.cat([m, r], dim=-1)


def folded_linear(x, wf, c1, b1, mean, rstd):
    """LayerNorm folded into a GEMM: rstd (x wf^T - mean c1) + b1, with wf = gamma (.) W, c1 = column sums of wf, b1 = beta . W^T (+ bias)."""
    return rstd * (x @ wf.T - mean * c1) + b1


# ---- attention ----------------------------------------------------------------------------------------------------------------------------------
def split_qkv(qkv, B, N):
    d = qkv.shape[-1] // 3
    return tuple(t.reshape(B, N, d) for t in qkv.split(d, dim=-1))


def attn_model(q, k, v, H):
    """Self-attention as the kernels compute it (tld_attn_core.h:83-85, tld_attn.hip:197-199): p = exp(s - max) is rounded to bf16 for the
    P V product on the matrix pipe, the row sum is taken from the unrounded p in fp32."""
    qh, kh, vh = R._heads(q, H), R._heads(k, H), R._heads(v, H)
    s = qh @ kh.transpose(-1, -2) / math.sqrt(qh.shape[-1])
    p = torch.exp(s - s.amax(-1, keepdim=True))
    return R._merge((bf16(p) @ vh) / p.sum(-1, keepdim=True))


def cross_row(x_in, att, wq, bwq, v, noise_row, label_row, n2_unused=None):
    """The block's middle from the engine's tables: x1 = x + att; the cross-attention over the sample's two conditioning tokens is a sigmoid of
    the logit difference; returns (x1, x2 = x1 + cross).  x_in, att [B, N, d]; wq [T, H, d], bwq [T, H], v [T, d]; *_row [B] token rows."""
    B, N, d = x_in.shape
    H = wq.shape[1]
    x1 = x_in + att
    mean = x1.mean(-1, keepdim=True)
    c = x1 - mean
    rstd = 1.0 / torch.sqrt((c * c).mean(-1, keepdim=True) + EPS)
    dw = wq[label_row] - wq[noise_row]                                   # [B, H, d]
    dl = torch.einsum("bnd,bhd->bnh", c, dw) * rstd + (bwq[label_row] - bwq[noise_row])[:, None, :]
    pl = torch.sigmoid(dl)                                               # weight of the label token
    vn, vl = v[noise_row].view(B, 1, H, d // H), v[label_row].view(B, 1, H, d // H)
    cr = vn + pl[..., None] * (vl - vn)
    return x1, x1 + cr.reshape(B, N, d)


def cross_plain(w, i, x1, y2, H):
    """The same cross-attention from the weights: x1 [B, N, d], y2 [B, 2, d] (noise token, label token) -> x1 + CA(LN2 x1, y)."""
    p = f"{BLK}decoder_blocks.{i}."
    a2 = R.ln_fwd(x1, w[p + "norm2.weight"], w[p + "norm2.bias"])[0]
    qc = R.linear_fwd(a2, w[p + "cross_attention.q_linear.weight"])
    kv = R.linear_fwd(y2, w[p + "cross_attention.kv_linear.weight"])
    return x1 + R.cross_fwd(qc, kv, H)[0]


# ---- MLP ----------------------------------------------------------------------------------------------------------------------------------------
def gelu_poly_half(y):
    """GELU(2 y) as gelu_erf_fast2_half computes it (tld_common.h:100-115): erf(sqrt2 y) ~ clamp(y R(y^2), -1, 1), R of degree 6 in y^2."""
    u = y * y
    r = torch.full_like(u, 3.952182666e-04)
    for c in (-6.822538060e-03, 5.043737174e-02, -2.115262865e-01, 5.651242001e-01, -1.035131935e+00, 1.591872892e+00):
        r = r * u + c
    return y + y * (y * r).clamp(-1.0, 1.0)


def dw_gelu(h, dw_w, dw_b, G):
    """GELU(depthwise 3x3(h) + b): h [B, N, hid], dw_w [hid, 9], dw_b [hid]."""
    return R.gelu(R.dwconv_fwd(h, dw_w, dw_b, G))


def dw_gelu_model(h, dw_w, dw_b, G, taps_bf16):
    """The halved-table forms: y = conv(h; w / 2) + b / 2 (the halving is exact), GELU(2 y) by the degree-6 polynomial.  taps_bf16: the fused
    up-projection epilogues and the seam kernel hold the halved taps as bf16 (tld_engine.hip, dw_wpk); the tiled and streaming kernels in fp32."""
    wh = 0.5 * dw_w
    if taps_bf16:
        wh = bf16(wh)
    return gelu_poly_half(R.dwconv_fwd(h, wh, 0.5 * dw_b, G))


# ---- sampler ------------------------------------------------------------------------------------------------------------------------------------
def cfg_combine(out2b, g):
    """[2 B, ...] (conditional half first) -> g cond + (1 - g) uncond -- tld/diffusion.py:124-125."""
    B = out2b.shape[0] // 2
    return g * out2b[:B] + (1.0 - g) * out2b[B:]


def blend(m, a, b):
    return m * a + (1.0 - m) * b


def update(x_t, x0, x0_prev, co):
    """One multistep update: co = (sigma, a, b, c, c1, c2) of schedule.step_coefficients -- DPM-Solver++(2M) where c2 != 0, DDIM / the
    first-order first step where (c1, c2) = (1, 0)."""
    _, a, b, c, c1, c2 = (float(v) for v in co)
    D = c1 * x0 - c2 * x0_prev
    return (a * D + b * x_t) / c


def update_from(x_t, x0, x0_prev, co, s_next, eps, z0, mask):
    """update, then the inpainting blend at the next level: the kept region rides the forward process of the same eps."""
    xt = update(x_t, x0, x0_prev, co)
    return xt if mask is None else blend(mask, xt, s_next * eps + (1.0 - s_next) * z0)


def final_x0(x0, sharp, bright, z0=None, mask=None):
    x0 = x0.clone() if mask is None else blend(mask, x0, z0)
    x0[:, 3] += sharp
    x0[:, 0] += bright
    return x0


def start_mix(eps, z0, s0):
    return s0 * eps + (1.0 - s0) * z0


# ---- the chain (host check against the reference fixtures) ------------------------------------------------------------------------------------
def chain(cfg, w, x, sigma, label):
    """Every transition above in order, plain weights: (x0 [B, C, S, S], {stage: [B, N, d]}) with the stage names of the g1 fixture."""
    c = cfg if isinstance(cfg, dict) else cfg.__dict__
    d, L, patch, C = c["embed_dim"], c["n_layers"], c["patch_size"], c["n_channels"]
    H, G = d // 64, c["image_size"] // patch
    B = x.shape[0]
    st = {}
    pn, pl = cond_pre(w, sigma, label)
    y = cond_y(w, torch.cat([pn, pl]))                                    # the engine's row order: noise rows, then label rows
    st["cond_y"] = torch.stack([y[:B], y[B:]], dim=1)
    nr, lr = torch.arange(B), torch.arange(B) + B
    t = embed(w, x, patch)
    st["tokens0"] = t
    for i in range(L):
        p = f"{BLK}decoder_blocks.{i}."
        a1 = R.ln_fwd(t, w[p + "norm1.weight"], w[p + "norm1.bias"])[0]
        q, k, v = split_qkv(R.linear_fwd(a1, w[p + "self_attention.qkv_linear.weight"]), B, G * G)
        att = R.attn_fwd(q, k, v, H)
        kv, wq, bwq = cond_tables(w, y, i, H)
        x1, x2 = cross_row(t, att, wq, bwq, kv[:, d:], nr, lr)
        a3 = R.ln_fwd(x2, w[p + "norm3.weight"], w[p + "norm3.bias"])[0]
        h = R.linear_fwd(a3, w[p + "mlp.mlp.0.weight"].reshape(-1, d), w[p + "mlp.mlp.0.bias"])
        gl = dw_gelu(h, w[p + "mlp.mlp.1.weight"].reshape(-1, 9), w[p + "mlp.mlp.1.bias"], G)
        t = x2 + R.linear_fwd(gl, w[p + "mlp.mlp.3.weight"].reshape(d, -1), w[p + "mlp.mlp.3.bias"])
        if i == 0:
            st["blk0_sa"], st["blk0_ca"], st["blk0_mlp"] = x1, x2, t
            st["blk0_ca_plain"] = cross_plain(w, 0, x1, st["cond_y"], H)
    st["tokens_final"] = t
    return tail(w, t, C, patch), st

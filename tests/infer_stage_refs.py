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


# ---- MX-fp8 operands (the fp8 GEMM mode; tests/test_gpu_fp8_stages.py) ---------------------------------------------------------------------------
def _pow2(k):
    """2^k in float64 for an integer tensor k (|k| < 1023), built from the exponent field: exact on every device, where pow may round."""
    return ((k.long() + 1023) << 52).view(torch.float64)


def mx8_quantize(x):
    """x [R, K] (K % 32 == 0) -> (e4m3 codes [R, K], E8M0 bytes [R, K / 32]) as float64 byte values 0 ... 255, the form read_stage returns.
    OCP Microscaling v1.0 as tld_quant.hip states it: per 32-element block X = 2^(floor(log2 amax) - 8), q = e4m3_rne(clamp(v / X, -448, 448)).
    Integer arithmetic on any device -- no float8 type; tests/test_infer_stage_refs_host.py holds it bit for bit against
    mx8_emulation.mx8_quantize (which converts through torch.float8_e4m3fn)."""
    R_, K = x.shape
    xb = x.double().view(R_, K // 32, 32)
    amax = xb.abs().amax(-1)
    e = torch.frexp(amax)[1] - 1                                           # floor(log2 amax) for amax > 0
    e8 = torch.where(amax > 0, (e + 119).clamp(min=0), torch.zeros_like(e))
    v = (xb * _pow2(127 - e8)[..., None]).clamp(-448.0, 448.0)
    a = v.abs()
    ex = torch.where(a < 2.0 ** -6, torch.full_like(e8[..., None], -6), torch.frexp(a)[1] - 1)      # subnormals: multiples of 2^-9
    q = torch.round(a * _pow2(3 - ex))                 # nearest even, in units of 2^(ex - 3): 8 ... 16 (normal), 0 ... 8 (subnormal)
    code = (ex + 6) * 8 + q.long()                                         # ((ex + 7) << 3 | q - 8); q = 16 carries into the exponent by itself
    code = code + 128 * torch.signbit(v).long()
    return code.view(R_, K).double(), e8.double()


def mx8_dequantize(q, s):
    """Codes [R, K] and scale bytes [R, K / 32] (float byte values) -> float64 values."""
    c = q.long()
    ex, man = (c >> 3) & 15, c & 7
    mag = torch.where(ex > 0, (8 + man).double() * _pow2(ex - 10), man.double() * 2.0 ** -9)
    v = torch.where(c >= 128, -mag, mag)
    return (v.view(q.shape[0], -1, 32) * _pow2(s.long() - 127)[..., None]).view(q.shape)


def mx8_model(ref):
    """What an exact producer followed by one bf16 rounding and the quantiser would hand the GEMM: the yardstick of the producers' MODELLED class."""
    return mx8_dequantize(*mx8_quantize(bf16(ref)))


def mx8_linear(aq, as_, w, bias=None, resid=None):
    """The fp8 GEMM on the engine's operands: dequantised A [M, K] x dequantised weights as held w [N, K] (+ bias, + residual).  Exact in float64."""
    y = mx8_dequantize(aq, as_) @ w.T
    if bias is not None:
        y = y + bias
    return y if resid is None else y + resid


def mx8_first_difference(q, s, q_ref, s_ref):
    """(differing codes, differing scale bytes, description of the first differing (row, 32-block)) of two operands; ('', 0, 0) when bitwise equal."""
    dq, ds = q != q_ref, s != s_ref
    nq, ns = int(dq.sum()), int(ds.sum())
    if nq + ns == 0:
        return 0, 0, ""
    blk = dq.view(q.shape[0], -1, 32).any(-1) | ds
    r, b = (int(t[0]) for t in torch.nonzero(blk, as_tuple=True))
    kind = "scale" if bool(ds[r, b]) else "byte"
    return nq, ns, (f"first at (row {r}, block {b}): {kind} -- scale {int(s[r, b])} vs {int(s_ref[r, b])}, "
                    f"{int(dq[r, b * 32:(b + 1) * 32].sum())} of 32 codes differ")


def dw_partial_tile_mask(G):
    """Pixels [G, G] of the partial last 16 x 16 tiles of the tiled depthwise kernel (grids that are not a multiple of 16 wide: 24, 40 ...), or None."""
    if G % 16 == 0:
        return None
    yy, xx = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
    return (yy >= G - G % 16) | (xx >= G - G % 16)


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

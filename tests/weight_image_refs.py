"""Every weight image of the inference engine, restated in numpy, bit for bit.

The engine builds its images with the refresh kernels (csrc/tld_refresh.hip) and nothing else, so this file is what they are held against:
tests/test_gpu_weight_refresh.py reads every image through the stage hook and compares bits.  numpy only, importable without a GPU.

``weight_images(state_dict, cfg, mode)`` returns {stage name: array} for the images an engine of that mode holds, under the names of
include/tld_hip.h: fp32 images as float32, bf16 images as their uint16 bit patterns, e4m3 codes and E8M0 scales as uint8 (scales in logical
[rows, K / 32] order).  ``as_read`` turns one into the float32 array the stage hook returns for it.  ``engine_mode`` says which images
tld_engine_create / tld_engine_set_gemm_dtype choose for a configuration (the restatement lives in tests/body_plan_ref.py).
"""
import ctypes as C

import numpy as np

BLK = "denoiser_trans_block."


def _bf16_bits(x):
    """Round-to-nearest-even to bf16, as uint16 (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def _split_hl(w):
    """[2, ...]: hi = bf16(w), lo = bf16(w - float(hi)), the subtraction in fp32."""
    w = np.asarray(w, np.float32)
    hi = _bf16_bits(w)
    return np.stack([hi, _bf16_bits(w - _bf16_value(hi))])


def _reference(wout, wd, bd, bo):
    """out_proj folded into the last block's down projection (csrc/tld_tail_fold_math.h): W' [pd, hid], b' [pd], the split image [2, pdp, d + hid]."""
    pd, d = wout.shape
    hid = wd.shape[1]
    q = _bf16_value(_bf16_bits(wd)).astype(np.float64)
    w64 = wout.astype(np.float64)
    s = np.zeros((pd, hid), np.float64)
    sb = np.zeros(pd, np.float64)
    for k in range(d):                                   # the sequential sum: one product (exact in float64) and one add per k
        s += w64[:, k:k + 1] * q[k][None, :]
        sb += w64[:, k] * np.float64(bd[k])
    wf = s.astype(np.float32)
    bf = (sb + bo.astype(np.float64)).astype(np.float32)
    pdp, K = (pd + 15) // 16 * 16, d + hid
    row = np.concatenate([wout, wf], axis=1)
    hi = _bf16_bits(row)
    lo = _bf16_bits(row - _bf16_value(hi))               # fp32 subtraction, exact or rounded once as in the header
    img = np.zeros((2, pdp, K), np.uint16)
    img[0, :pd], img[1, :pd] = hi, lo
    return wf, bf, img


def ln_fold(w, gamma, beta, bias=None):
    """A LayerNorm folded into the Linear behind it: wf = bf16(gamma * W) with the product rounded to fp32 first, c1 = float32(sum_k float64(wf)),
    b1 = float32(sum_k float64(beta_k) * float64(W_nk) [+ bias]).  Both sums run k = 0 .. K - 1 with one add per element: cumsum, not the pairwise np.sum."""
    w = np.asarray(w, np.float32)
    wf = _bf16_bits(np.asarray(gamma, np.float32)[None, :] * w)
    c1 = np.cumsum(_bf16_value(wf).astype(np.float64), axis=1)[:, -1].astype(np.float32)
    sb = np.cumsum(np.asarray(beta, np.float32).astype(np.float64)[None, :] * w.astype(np.float64), axis=1)[:, -1]
    if bias is not None:
        sb = sb + np.asarray(bias, np.float32).astype(np.float64)
    return wf, c1, sb.astype(np.float32)


def packed_rows(d):
    """dst[src]: where row src of [q; k; v] x [head][64] sits in the fused QKV -> attention kernel's [head][feature half][q | k | v][32] order."""
    src = np.arange(3 * d)
    part, h, c = src // d, (src % d) // 64, src % 64
    return h * 192 + (c >> 5) * 96 + part * 32 + (c & 31)


def dw_images(w, b):
    """Depthwise taps [hid, 1, 3, 3] and bias [hid] -> the taps [9, hid], their halves, the halved bias, and the halved taps as bf16 pairs
    [3, 4, hid, 2] (low half first): per window row du with taps (w0, w1, w2), kind 0 = (0, w0), 1 = (w1, w2), 2 = (w0, w1), 3 = (w2, 0)."""
    w9c = np.ascontiguousarray(np.asarray(w, np.float32).reshape(-1, 9).T)
    half = w9c * np.float32(0.5)
    h = _bf16_bits(half).reshape(3, 3, -1)
    z = np.zeros_like(h[:, 0])
    pk = np.stack([np.stack([z, h[:, 0]], -1), np.stack([h[:, 1], h[:, 2]], -1), np.stack([h[:, 0], h[:, 1]], -1), np.stack([h[:, 2], z], -1)], axis=1)
    return w9c, half, np.asarray(b, np.float32) * np.float32(0.5), pk


def quant_mx8(w):
    """fp32 [rows, K] -> e4m3 codes [rows, K] and E8M0 scales [rows, K / 32] through the library's host quantiser (tld_debug_quant_mx8_host: no device)."""
    from transformer_latent_diffusion_amd import _lib
    w = np.ascontiguousarray(w, np.float32)
    rows, K = w.shape
    q, s = np.zeros((rows, K), np.uint8), np.zeros((K // 128, rows, 4), np.uint8)
    _lib.check(_lib.lib().tld_debug_quant_mx8_host(w.ctypes.data_as(C.POINTER(C.c_float)), rows, K, q.ctypes.data, s.ctypes.data), "quant_mx8_host")
    return q, np.ascontiguousarray(s.transpose(1, 0, 2)).reshape(rows, K // 32)


def dequant_mx8(q, s):
    """code x 2^(scale - 127) as float32 (exact): what the hook returns for an fp8 weight."""
    ex, man = ((q >> 3) & 15).astype(np.int32), (q & 7).astype(np.float32)
    mag = np.where(ex > 0, np.ldexp(np.float32(8) + man, ex - 10), np.ldexp(man, -9)).astype(np.float32)
    return np.ldexp(np.where(q & 0x80, -mag, mag), np.repeat(s.astype(np.int32), 32, axis=1) - 127).astype(np.float32)


def engine_mode(cfg, env=None, gemm_dtype="bf16"):
    """Which images an engine holds (tld_engine_create with the switches in ``env``, then tld_engine_set_gemm_dtype): the plan of body_plan_ref.py."""
    import body_plan_ref as B
    fp8 = gemm_dtype == "fp8"
    p = B.plan(B.shape(cfg), B.switches(env), fp8, 0, 1, 256)
    return dict(fp8=fp8, fold_ln1=p.fold_ln1, fold_ln3=p.fold_ln3, fold_tail=p.fold_tail_held, packed_qkv=p.fused_qa)


# stage name of an fp32 copy outside the blocks -> state_dict key
_GLOBAL_F32 = {
    "img.angular": "fourier_feats.0.angular_speeds", "img.ff1_w": "fourier_feats.1.weight", "img.ff1_b": "fourier_feats.1.bias",
    "img.ff3_w": "fourier_feats.3.weight", "img.ff3_b": "fourier_feats.3.bias", "img.label_w": "label_proj.weight", "img.label_b": "label_proj.bias",
    "img.norm_w": "norm.weight", "img.norm_b": "norm.bias", "img.conv_w": BLK + "patchify_and_embed.0.weight", "img.conv_b": BLK + "patchify_and_embed.0.bias",
    "img.pln1_w": BLK + "patchify_and_embed.2.weight", "img.pln1_b": BLK + "patchify_and_embed.2.bias", "img.plin_b": BLK + "patchify_and_embed.3.bias",
    "img.pln2_w": BLK + "patchify_and_embed.4.weight", "img.pln2_b": BLK + "patchify_and_embed.4.bias", "img.pos": BLK + "pos_embed.weight",
    "img.out_w": BLK + "out_proj.0.weight", "img.out_b": BLK + "out_proj.0.bias",
}
# ... and of one inside a block -> key behind "denoiser_trans_block.decoder_blocks.<i>."
_BLOCK_F32 = {
    "img.kv_w": "cross_attention.kv_linear.weight", "img.q_w": "cross_attention.q_linear.weight", "img.up_b": "mlp.mlp.0.bias", "img.dw_b": "mlp.mlp.1.bias",
    "img.down_b": "mlp.mlp.3.bias", "img.n1_w": "norm1.weight", "img.n1_b": "norm1.bias", "img.n2_w": "norm2.weight", "img.n2_b": "norm2.bias",
    "img.n3_w": "norm3.weight", "img.n3_b": "norm3.bias",
}

# every img.* stage name of include/tld_hip.h: outside the blocks, and behind "blk<i>."
GLOBAL_IMAGES = list(_GLOBAL_F32) + ["img.out_w_hl", "img.plin_w_hl", "img.plin_wt", "img.out_fold_hl", "img.out_fold_b"]
BLOCK_IMAGES = list(_BLOCK_F32) + ["img." + n for n in ("qkv_wf qkv_c1 qkv_b1 qkv_wp qkv_c1p qkv_b1p dw_w9c dw_w9c_half dw_b_half dw_wpk qkv_w8 qkv_s8 up_w8 up_s8 "
                                                         "down_w8 down_s8").split()]


def weight_images(state_dict, cfg, mode):
    sd = {k: np.asarray(v) for k, v in state_dict.items()}
    f32 = lambda k: np.ascontiguousarray(sd[k], dtype=np.float32)
    d, L, hid = cfg.embed_dim, cfg.n_layers, cfg.mlp_multiplier * cfg.embed_dim
    pd = cfg.n_channels * cfg.patch_size ** 2
    flat2 = lambda a: a if a.ndim == 1 else a.reshape(a.shape[0], -1)          # (conv weights [n, c, kh, kw] are held as [n, c kh kw])
    out = {name: flat2(f32(key)) for name, key in _GLOBAL_F32.items()}
    wout, plin = f32(BLK + "out_proj.0.weight"), f32(BLK + "patchify_and_embed.3.weight")
    out["img.out_w_hl"] = _split_hl(wout)                                    # [2, pd, d]
    out["img.plin_w_hl"] = _split_hl(plin)                                   # [2, d, pd]
    out["img.plin_wt"] = np.ascontiguousarray(plin.T)                        # [d, pd] -> [pd, d]
    for i in range(L):
        b = f"{BLK}decoder_blocks.{i}."
        n = lambda s: f"blk{i}.{s}"
        for name, key in _BLOCK_F32.items():
            out[n(name)] = flat2(f32(b + key))
        wqkv, wup, wdown = f32(b + "self_attention.qkv_linear.weight"), f32(b + "mlp.mlp.0.weight").reshape(hid, d), f32(b + "mlp.mlp.3.weight").reshape(d, hid)
        if mode["fp8"]:
            for nm, w in (("qkv", wqkv), ("up", wup), ("down", wdown)):
                q, s = quant_mx8(w)
                out[n(f"img.{nm}_w8")], out[n(f"img.{nm}_s8")] = q, s
                out[n("w" + nm)] = dequant_mx8(q, s)
        else:
            out[n("wdown")] = _bf16_bits(wdown)
        if mode["fold_ln1"]:
            wf, c1, b1 = ln_fold(wqkv, f32(b + "norm1.weight"), f32(b + "norm1.bias"))
            out[n("wqkv")], out[n("qkv_c1")], out[n("qkv_b1")] = wf, c1, b1      # (read in logical order whatever the storage)
            out[n("img.qkv_wf")], out[n("img.qkv_c1")], out[n("img.qkv_b1")] = wf, c1, b1
            if mode["packed_qkv"]:
                dst = packed_rows(d)
                for nm, a in (("img.qkv_wp", wf), ("img.qkv_c1p", c1), ("img.qkv_b1p", b1)):
                    p = np.empty_like(a)
                    p[dst] = a
                    out[n(nm)] = p
        elif not mode["fp8"]:
            out[n("wqkv")] = _bf16_bits(wqkv)
        if mode["fold_ln3"]:
            out[n("wup")], out[n("up_c1")], out[n("up_b1")] = ln_fold(wup, f32(b + "norm3.weight"), f32(b + "norm3.bias"), f32(b + "mlp.mlp.0.bias"))
        elif not mode["fp8"]:
            out[n("wup")] = _bf16_bits(wup)
        out[n("img.dw_w9c")], out[n("img.dw_w9c_half")], out[n("img.dw_b_half")], out[n("img.dw_wpk")] = dw_images(f32(b + "mlp.mlp.1.weight"), f32(b + "mlp.mlp.1.bias"))
    if mode["fold_tail"]:
        b = f"{BLK}decoder_blocks.{L - 1}."
        _, bf, img = _reference(wout, f32(b + "mlp.mlp.3.weight").reshape(d, hid), f32(b + "mlp.mlp.3.bias"), f32(BLK + "out_proj.0.bias"))
        out["img.out_fold_hl"], out["img.out_fold_b"] = img, bf
    assert wout.shape == (pd, d)
    return out


def as_read(a):
    """The float32 array the stage hook returns for an image: bf16 bit patterns as their values, bytes as 0 .. 255."""
    if a.dtype == np.uint16:
        return _bf16_value(a)
    return np.ascontiguousarray(a, dtype=np.float32)

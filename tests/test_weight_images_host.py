"""CPU: the numpy restatement of the engine's weight images (tests/weight_image_refs.py) -- what can be held without a device.  The bits themselves are
held against the engine in tests/test_gpu_weight_refresh.py."""
import numpy as np
import pytest

from transformer_latent_diffusion_amd import DenoiserConfig, weights
from weight_image_refs import BLOCK_IMAGES, GLOBAL_IMAGES, _bf16_bits, _bf16_value, as_read, dequant_mx8, dw_images, engine_mode, packed_rows, quant_mx8, weight_images


def _cfg(d, image, patch=2):
    return DenoiserConfig(image_size=image, noise_embed_dims=256, patch_size=patch, embed_dim=d, dropout=0, n_layers=2, text_emb_size=768, n_channels=4)


CONFIGS = {"d192_patch4": _cfg(192, 32, 4), "d192_patch1": _cfg(192, 8, 1), "d256_64tok": _cfg(256, 16)}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_shapes_and_dtypes(name):
    cfg = CONFIGS[name]
    d, hid, pd, ntok = cfg.embed_dim, 4 * cfg.embed_dim, 4 * cfg.patch_size ** 2, (cfg.image_size // cfg.patch_size) ** 2
    mode = engine_mode(cfg)
    assert mode == dict(fp8=False, fold_ln1=False, fold_ln3=d == 256, fold_tail=True, packed_qkv=False)
    sd = weights.synth_state_dict(cfg, 1)
    im = weight_images(sd, cfg, mode)
    want = {"img.angular": (np.float32, (128,)), "img.ff1_w": (np.float32, (d, 256)), "img.conv_w": (np.float32, (pd, pd)), "img.pos": (np.float32, (ntok, d)),
            "img.out_w": (np.float32, (pd, d)), "img.out_b": (np.float32, (pd,)), "img.out_w_hl": (np.uint16, (2, pd, d)), "img.plin_w_hl": (np.uint16, (2, d, pd)),
            "img.plin_wt": (np.float32, (pd, d)), "img.out_fold_hl": (np.uint16, (2, (pd + 15) // 16 * 16, d + hid)), "img.out_fold_b": (np.float32, (pd,)),
            "blk1.img.kv_w": (np.float32, (2 * d, d)), "blk1.img.up_b": (np.float32, (hid,)), "blk0.wqkv": (np.uint16, (3 * d, d)), "blk0.wup": (np.uint16, (hid, d)),
            "blk1.wdown": (np.uint16, (d, hid)), "blk0.img.dw_w9c": (np.float32, (9, hid)), "blk0.img.dw_w9c_half": (np.float32, (9, hid)),
            "blk0.img.dw_b_half": (np.float32, (hid,)), "blk1.img.dw_wpk": (np.uint16, (3, 4, hid, 2))}
    if d == 256:
        want.update({"blk0.up_c1": (np.float32, (hid,)), "blk1.up_b1": (np.float32, (hid,))})
    for n, (dt, shape) in want.items():
        assert im[n].dtype == dt and im[n].shape == shape, (n, im[n].dtype, im[n].shape)
    assert ("blk0.up_c1" in im) == (d == 256) and "blk0.qkv_c1" not in im and "blk0.img.qkv_wp" not in im
    names = set(GLOBAL_IMAGES) | {f"blk{i}.{n}" for i in range(2) for n in BLOCK_IMAGES + ["wqkv", "wup", "wdown", "qkv_c1", "qkv_b1", "up_c1", "up_b1"]}
    assert set(im) <= names                                                    # nothing the stage hook has no name for
    assert all(as_read(a).dtype == np.float32 and as_read(a).shape == a.shape for a in im.values())
    assert np.array_equal(im["img.plin_wt"], sd["denoiser_trans_block.patchify_and_embed.3.weight"].T)
    # each lo half of a hi / lo split is bf16(w - hi), and hi + lo keeps 16 significant bits
    for n, key in (("img.out_w_hl", "out_proj.0.weight"), ("img.plin_w_hl", "patchify_and_embed.3.weight")):
        w = sd["denoiser_trans_block." + key]
        hi, lo = im[n]
        assert np.array_equal(hi, _bf16_bits(w)) and np.array_equal(lo, _bf16_bits(w - _bf16_value(hi)))
        assert np.all(np.abs(_bf16_value(hi).astype(np.float64) + _bf16_value(lo) - w) <= 2.0 ** -16 * np.abs(w))
    fold = im["img.out_fold_hl"]
    assert not fold[:, pd:].any() and np.array_equal(fold[0, :pd, :d], im["img.out_w_hl"][0]) and np.array_equal(fold[1, :pd, :d], im["img.out_w_hl"][1])


def test_folds_and_packed_rows_at_the_flagship_width():
    cfg = _cfg(768, 32)
    d = 768
    assert engine_mode(cfg) == dict(fp8=False, fold_ln1=True, fold_ln3=True, fold_tail=True, packed_qkv=True)
    assert engine_mode(cfg, {"TLD_FUSE_QKV_ATTN": "0"})["packed_qkv"] is False and engine_mode(cfg, {"TLD_FOLD_LN1": "0"})["packed_qkv"] is False
    assert engine_mode(cfg, gemm_dtype="fp8") == dict(fp8=True, fold_ln1=False, fold_ln3=False, fold_tail=False, packed_qkv=False)
    dst = packed_rows(d)
    assert np.array_equal(np.sort(dst), np.arange(3 * d))                      # a bijection of the 3 d rows
    assert dst[0] == 0 and dst[32] == 96 and dst[d] == 32 and dst[2 * d + 33] == 96 + 64 + 1 and dst[64] == 192      # q0, q32, k0, v33 of head 0; q0 of head 1
    sd = weights.synth_state_dict(cfg, 1)
    im = weight_images(sd, cfg, engine_mode(cfg))
    wf, wp = im["blk1.img.qkv_wf"], im["blk1.img.qkv_wp"]
    assert np.array_equal(wp[dst], wf) and np.array_equal(im["blk1.img.qkv_c1p"][dst], im["blk1.qkv_c1"]) and np.array_equal(im["blk1.wqkv"], wf)
    w = sd["denoiser_trans_block.decoder_blocks.1.self_attention.qkv_linear.weight"]
    g, be = sd["denoiser_trans_block.decoder_blocks.1.norm1.weight"], sd["denoiser_trans_block.decoder_blocks.1.norm1.bias"]
    assert np.array_equal(wf, _bf16_bits(g[None, :] * w))
    # the float32 sums are the float64 ones to rounding: 2^-24 relative of the sum of magnitudes covers any order
    c64, b64 = _bf16_value(wf).astype(np.float64).sum(1), (be.astype(np.float64) * w).sum(1)
    assert np.all(np.abs(im["blk1.qkv_c1"] - c64) <= 2.0 ** -23 * np.abs(_bf16_value(wf)).sum(1))
    assert np.all(np.abs(im["blk1.qkv_b1"] - b64) <= 2.0 ** -23 * np.abs(be * w).sum(1))


def test_tap_kinds_on_a_hand_written_window():
    taps = np.arange(1, 10, dtype=np.float32).reshape(1, 1, 3, 3) * np.float32(2)          # halves 1 .. 9: exact in bf16
    w9c, half, bh, pk = dw_images(np.concatenate([taps, -taps]), np.array([3.0, -5.0], np.float32))
    assert np.array_equal(w9c[:, 0], np.arange(1, 10) * 2.0) and np.array_equal(w9c[:, 1], -w9c[:, 0])
    assert np.array_equal(half, w9c / 2) and np.array_equal(bh, [1.5, -2.5])
    v = _bf16_value(pk)                                                        # [3, 4, 2, 2]: (window row, kind, channel, half of the pair)
    for du in range(3):
        w0, w1, w2 = 3 * du + 1.0, 3 * du + 2.0, 3 * du + 3.0
        assert v[du, :, 0].tolist() == [[0, w0], [w1, w2], [w0, w1], [w2, 0]]
        assert v[du, :, 1].tolist() == [[0, -w0], [-w1, -w2], [-w0, -w1], [-w2, 0]]
    assert not pk[:, 0, :, 0].any() and not pk[:, 3, :, 1].any()               # the zero halves are +0 bits


def test_fp8_images_through_the_host_quantiser():
    cfg = _cfg(256, 16)
    sd = weights.synth_state_dict(cfg, 1)
    im = weight_images(sd, cfg, engine_mode(cfg, gemm_dtype="fp8"))
    d, hid = 256, 1024
    for nm, (rows, K), key in (("qkv", (3 * d, d), "self_attention.qkv_linear.weight"), ("up", (hid, d), "mlp.mlp.0.weight"), ("down", (d, hid), "mlp.mlp.3.weight")):
        q, s, deq = im[f"blk0.img.{nm}_w8"], im[f"blk0.img.{nm}_s8"], im[f"blk0.w{nm}"]
        assert q.dtype == s.dtype == np.uint8 and q.shape == (rows, K) and s.shape == (rows, K // 32) and deq.dtype == np.float32 and deq.shape == (rows, K)
        w = sd["denoiser_trans_block.decoder_blocks.0." + key].reshape(rows, K)
        q2, s2 = quant_mx8(w)
        assert np.array_equal(q, q2) and np.array_equal(s, s2) and np.array_equal(deq, dequant_mx8(q, s))
        # the scale is 2^(floor(log2 amax) - 8) per block of 32; the dequantised weight is within 2^-3 relative of the weight (half an e4m3 step is 2^-4;
        # a scaled value in (448, 512) saturates at 448, at most 64 / 512 away), or half a subnormal step 2^-10 of the scale
        amax = np.abs(w).reshape(rows, K // 32, 32).max(-1)
        assert np.array_equal(s.astype(np.int32) - 127, np.floor(np.log2(amax)).astype(np.int32) - 8)
        step = np.repeat(np.exp2(s.astype(np.float64) - 127), 32, axis=1)
        assert np.all(np.abs(deq - w) <= np.maximum(2.0 ** -3 * np.abs(w), 2.0 ** -10 * step))
    assert "blk0.img.qkv_wf" not in im and "img.out_fold_hl" not in im and "blk0.up_c1" not in im

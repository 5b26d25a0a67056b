"""CPU: the stage hook's decoder (decode_stage in csrc/tld_stages.h, behind every tld_*_read_stage) through tld_debug_decode_stage, against a few lines
of numpy each.  Every conversion is exact, so every comparison is on bit patterns."""
import ctypes as C

import numpy as np

from transformer_latent_diffusion_amd import _lib

F32, BF16, U8, MX8S, MX8W = range(5)
PLAIN, QKV_ROWS, NHWC = range(3)
TLD_ERR_INVALID, TLD_ERR_SHAPE = 1, 3


def _decode(raw, dtype, shape, layout=PLAIN, aux=None, outer_stride=0, d=0, heads=0, numel=None, status=0):
    shape4 = (C.c_int64 * 4)(*(list(shape) + [1] * (4 - len(shape))))
    n = int(np.prod(shape))
    out = np.full(n, -7.0, np.float32)
    rc = _lib.lib().tld_debug_decode_stage(raw.ctypes.data if raw is not None else None, aux.ctypes.data if aux is not None else None, dtype, layout, shape4,
                                           outer_stride, d, heads, out.ctypes.data_as(C.POINTER(C.c_float)), n if numel is None else numel)
    assert rc == status, (rc, _lib.lib().tld_last_error())
    return out.reshape(shape)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _widen(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def _e4m3(q):
    q = q.astype(np.int64)
    ex, man = (q >> 3) & 15, q & 7
    mag = np.where(ex > 0, (8 + man) * 2.0 ** (ex - 10), man * 2.0 ** -9)
    return np.where(q & 0x80, -mag, mag)


def test_bf16_plain_is_the_upper_half_of_the_word():
    h = np.array([0x0000, 0x8000, 0x7FC1, 0xFFFF, 0x7F7F, 0xFF7F, 0x0001, 0x3F80, 0xC2F7, 0x7F80], np.uint16)       # +-0, two NaN patterns, +-largest finite, ...
    assert _same_bits(_decode(h, BF16, (2, 5)), _widen(h).reshape(2, 5))
    rng = np.random.default_rng(0)
    h = rng.integers(0, 1 << 16, 3 * 7 * 2, dtype=np.uint16)
    assert _same_bits(_decode(h, BF16, (3, 7, 2)), _widen(h).reshape(3, 7, 2))
    f = rng.standard_normal(11).astype(np.float32)
    assert _same_bits(_decode(f, F32, (11,)), f)


def test_bytes_and_the_scale_layout():
    b = np.arange(256, dtype=np.uint8)[::-1].copy()
    assert _same_bits(_decode(b, U8, (4, 64)), b.astype(np.float32).reshape(4, 64))
    rows, cols = 3, 8
    stored = np.random.default_rng(1).integers(0, 256, (cols // 4, rows, 4), dtype=np.uint8)                       # [cols / 4][rows][4]
    assert _same_bits(_decode(stored, MX8S, (rows, cols)), stored.transpose(1, 0, 2).reshape(rows, cols).astype(np.float32))


def test_fp8_weights_are_dequantised_with_every_code_and_scale():
    rows, cols = 2, 128
    q = np.random.default_rng(2).permutation(256).astype(np.uint8).reshape(rows, cols)                            # all 256 e4m3 codes
    sc = np.array([[[127, 0, 130, 120], [97, 127, 0, 140]]], np.uint8)                                             # [cols / 128][rows][4]
    e8 = np.repeat(sc[0], 32, axis=1).astype(np.int64)                                                             # [rows][cols]: one scale per 32 columns
    want = (_e4m3(q) * 2.0 ** (e8 - 127)).astype(np.float32)
    assert np.isfinite(want).all() and (want[e8 == 0] != 0).sum() > 0
    assert _same_bits(_decode(q, MX8W, (rows, cols), aux=sc), want)


def test_nhwc_and_the_packed_qkv_rows_are_undone():
    B, Cc, H, W = 2, 3, 2, 2
    h = np.random.default_rng(3).integers(0, 1 << 16, (B, H, W, Cc), dtype=np.uint16)
    assert _same_bits(_decode(h, BF16, (B, Cc, H, W), layout=NHWC), _widen(h).transpose(0, 3, 1, 2))
    d, heads, row = 128, 2, 2
    packed = np.random.default_rng(4).standard_normal((3 * d, row)).astype(np.float32)
    want = np.empty_like(packed)
    for hd in range(heads):
        for part in range(3):
            for c in range(64):
                want[part * d + hd * 64 + c] = packed[hd * 192 + (c >> 5) * 96 + part * 32 + (c & 31)]
    assert _same_bits(_decode(packed, F32, (3 * d, row), layout=QKV_ROWS, d=d, heads=heads), want)
    hp = np.random.default_rng(5).integers(0, 1 << 16, (3 * d, row), dtype=np.uint16)
    wp = _widen(hp)
    for hd in range(heads):
        for part in range(3):
            for c in range(64):
                want[part * d + hd * 64 + c] = wp[hd * 192 + (c >> 5) * 96 + part * 32 + (c & 31)]
    assert _same_bits(_decode(hp, BF16, (3 * d, row), layout=QKV_ROWS, d=d, heads=heads), want)


def test_an_outer_stride_skips_the_pitch():
    shape, stride = (2, 3, 4, 1), 20
    f = np.random.default_rng(6).standard_normal(stride + 12).astype(np.float32)
    want = np.stack([f[:12], f[stride:stride + 12]]).reshape(shape)
    assert _same_bits(_decode(f, F32, shape, outer_stride=stride), want)
    h = np.random.default_rng(7).integers(0, 1 << 16, stride + 12, dtype=np.uint16)
    assert _same_bits(_decode(h, BF16, shape, outer_stride=stride), np.stack([_widen(h[:12]), _widen(h[stride:stride + 12])]).reshape(shape))


def test_refusals_leave_the_buffer_alone_and_say_why():
    L = _lib.lib()
    f = np.arange(12, dtype=np.float32)
    out = _decode(f, F32, (3, 4), numel=11, status=TLD_ERR_SHAPE)
    assert (out == -7.0).all() and b"12 elements" in L.tld_last_error()
    out = _decode(None, F32, (3, 4), status=TLD_ERR_INVALID)
    assert (out == -7.0).all() and b"null" in L.tld_last_error()
    q = np.zeros((2, 128), np.uint8)
    out = _decode(q, MX8W, (2, 128), aux=None, status=TLD_ERR_INVALID)                                            # fp8 weights without their scales
    assert (out == -7.0).all() and b"null" in L.tld_last_error()
    out = _decode(f, F32, (3, 4), layout=QKV_ROWS, d=128, heads=2, status=TLD_ERR_INVALID)                        # 3 rows are not 3 d
    assert (out == -7.0).all() and b"3 d" in L.tld_last_error()

"""CPU: the host side of the device batch preparation -- the numpy statement of its generator against the published
Philox known answers and against csrc/tld_batch_math.h built by the host compiler, the Beta method's distribution, the quantisation helpers
and the dataset's table, and the refusals of the C entry (all before any HIP call)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import batch_prep_ref as R
from transformer_latent_diffusion_amd import DeviceLatentDataset, _lib, dequantize_latents, quantize_latents

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = (((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"))
KS_ALPHA_001 = 1.95                      # the alpha = 0.001 critical value of sqrt(n) D_n


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_reference_philox_reproduces_the_published_known_answers():
    for ctr, key, want in KAT:
        assert _hex(R.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))) == want
    got = R.philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint32), np.array([k[1] for k in KAT], dtype=np.uint32))       # vectorised
    assert [_hex(r) for r in got] == [k[2] for k in KAT]


@pytest.fixture(scope="module")
def math_exe(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    exe = str(tmp_path_factory.mktemp("batch_math") / "batch_math_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "batch_math_main.cpp"), "-o", exe], check=True)
    return exe


def test_host_build_of_the_math_header_gives_the_known_answers(math_exe):
    out = subprocess.run([math_exe, "kat"], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    assert out[:3] == [k[2] for k in KAT]


@pytest.mark.parametrize("seed,step,replica", [(1234, 7, 0), (0xFEDCBA9876543210, (5 << 32) | 9, 3)])
def test_host_build_of_the_math_header_equals_the_numpy_reference(math_exe, seed, step, replica):
    n = 1500                                                           # x 4 groups = 6000 counters, every word and every conversion of each
    out = subprocess.run([math_exe, hex(seed), hex(step), str(replica), str(n)], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    rows = [l.split() for l in out if l]
    assert len(rows) == 4 * n
    streams = np.array([int(r[0]) for r in rows])
    c0 = np.array([int(r[1]) for r in rows], dtype=np.uint64)
    words = np.array([[int(x, 16) for x in r[2:6]] for r in rows], dtype=np.uint32)
    u32 = np.array([[int(x, 16) for x in r[6:18]] for r in rows], dtype=np.uint32)
    u64 = np.array([[int(x, 16) for x in r[18:20]] for r in rows], dtype=np.uint64)
    assert set(streams) == {0, 1, 2} and int(c0.max()) == 0xFFFFFFFF
    want = np.empty_like(words)
    for s in (0, 1, 2):
        want[streams == s] = R.batch_philox(seed, step, replica, s, c0[streams == s])
    assert np.array_equal(words, want)
    assert np.array_equal(u32[:, 0::3], R.uniform24_open(want).view(np.uint32))
    assert np.array_equal(u32[:, 1::3], R.uniform24(want).view(np.uint32))
    assert np.array_equal(u32[:, 2::3], R.uniform24_open_complement(want).view(np.uint32))
    upper = (want >> np.uint32(8)) >= (1 << 23)                         # where fp32 cannot hold u, it holds 1 - u: both halves are exact somewhere
    exact = ((want >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    assert upper.any() and (~upper).any()
    assert np.array_equal(R.uniform24_open_complement(want).astype(np.float64)[upper], (1.0 - exact)[upper])
    assert np.array_equal(R.uniform24_open(want).astype(np.float64)[~upper], exact[~upper])
    assert np.array_equal(u64[:, 0], R.uniform53_open(want[:, 0], want[:, 1]).view(np.uint64))
    assert np.array_equal(u64[:, 1], R.uniform32_open(want[:, 2]).view(np.uint64))


def test_uniform_conversions_at_their_ends():
    ends = np.array([0, 0xFF, 0x100, 0x7FFFFFFF, 0x80000000, 0xFFFFFEFF, 0xFFFFFFFF], dtype=np.uint32)
    uo, u = R.uniform24_open(ends), R.uniform24(ends)
    assert uo.dtype == u.dtype == np.float32
    assert uo.min() == np.float32(2.0 ** -25) and uo.max() == 1.0 and (uo > 0).all()          # never 0: the logarithm is finite, radius <= 5.89
    assert u.min() == 0.0 and u.max() == np.float32(1 - 2.0 ** -24)
    assert np.sqrt(-2 * np.log(float(uo.min()))) < 5.9
    d = R.uniform53_open(np.array([0, 0xFFFFFFFF], dtype=np.uint32), np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert d[0] == 2.0 ** -54 and d[1] == 1.0
    assert R.uniform32_open(np.array([0, 0xFFFFFFFF], dtype=np.uint32)).tolist() == [2.0 ** -33, 1 - 2.0 ** -33]


def _ks(sample, cdf):
    x = np.sort(np.asarray(sample, dtype=np.float64))
    n = x.size
    f = cdf(x)
    return max(float((np.arange(1, n + 1) / n - f).max()), float((f - np.arange(n) / n).max()))


def test_reference_normals_and_mask_stay_inside_the_bounds_the_device_is_held_to():
    from scipy import stats
    n = 1 << 20
    d = _ks(R.noise_f64(1234, 7, 0, n), stats.norm.cdf)
    print(f"normals: KS {d:.3e} against {KS_ALPHA_001 / np.sqrt(n):.3e}")
    assert d <= KS_ALPHA_001 / np.sqrt(n)
    m = 65536
    frac = float(R.label_mask(1234, 7, 0, m, 0.15).mean())
    print(f"dropout fraction {frac:.4f}")
    assert abs(frac - 0.15) <= 4 * np.sqrt(0.15 * 0.85 / m)


@pytest.mark.parametrize("a,b", [(1, 2.5), (0.5, 0.5), (2, 5), (0.25, 8)])
def test_reference_beta_method_stays_inside_the_ks_bound(a, b):
    from scipy import stats
    n = 65536
    nl, exhausted = R.noise_level(1234, 7, 0, n, a, b, return_exhausted=True)
    d = _ks(nl, stats.beta(a, b).cdf)
    print(f"Beta({a}, {b}): KS {d:.3e} against {KS_ALPHA_001 / np.sqrt(n):.3e}; draws that used up their attempts: {exhausted}")
    assert exhausted == 0 and (nl >= 0).all() and (nl <= 1).all()
    assert d <= KS_ALPHA_001 / np.sqrt(n)


def test_reference_beta_survives_tiny_and_large_shapes():
    for a, b in ((1e-3, 1e-3), (1e-3, 50.0), (300.0, 0.01), (40.0, 60.0)):
        nl = R.noise_level(5, 0, 0, 4096, a, b)
        assert np.isfinite(nl).all() and (nl >= 0).all() and (nl <= 1).all(), (a, b)
        assert abs(nl.mean() - a / (a + b)) < 5 * np.sqrt(a * b / ((a + b) ** 2 * (a + b + 1)) / 4096) + 1e-12, (a, b, nl.mean())


# ---- quantisation helpers and the dataset's table -------------------------------------------------------------------------------------------------
def _ref_quantize(lat, clip_val=20):                    # the formulas of tld/data.py:52-60, evaluated with torch on the CPU
    lat_norm = lat.clip(-clip_val, clip_val) / clip_val
    return (((lat_norm + 1) / 2) * 255).to(torch.uint8)


def _ref_dequantize(lat, clip_val=20):
    lat_norm = (lat.to(torch.float16) / 255) * 2 - 1
    return lat_norm * clip_val


@pytest.mark.parametrize("clip_val", [20, 7.5])
def test_quantisation_helpers_follow_the_reference_and_round_trip_every_code(clip_val):
    codes = torch.arange(256, dtype=torch.uint8)
    deq = dequantize_latents(codes, clip_val)
    assert deq.dtype == torch.float16 and torch.equal(deq, _ref_dequantize(codes, clip_val))
    lat = torch.randn(3, 4, 8, 8, generator=torch.Generator().manual_seed(1)) * clip_val * 0.6          # some beyond the clip
    q = quantize_latents(lat, clip_val)
    assert q.dtype == torch.uint8 and torch.equal(q, _ref_quantize(lat, clip_val))
    # a code's value is the lower edge of its cell up to fp16 rounding; half a cell above it, quantisation (which truncates) returns the code
    centres = deq.float() + clip_val / 255.0
    assert torch.equal(quantize_latents(centres, clip_val)[:255], codes[:255]) and int(quantize_latents(centres, clip_val)[255]) == 255
    assert float(deq[0]) == -clip_val and float(deq[255]) == clip_val


@pytest.mark.parametrize("clip_val,scale", [(20, 8), (7.5, 8), (20, 5.489)])
def test_dataset_table_is_the_dequantised_codes_over_the_scale_factor(clip_val, scale):
    lat = torch.randint(0, 256, (6, 4, 4, 4), dtype=torch.uint8)
    ds = DeviceLatentDataset(lat, torch.zeros(6, 10, dtype=torch.float16), clip_val=clip_val, vae_scale_factor=scale, device="cpu")
    want = _ref_dequantize(torch.arange(256), clip_val).float() / scale
    assert ds.table.dtype == torch.float32 and torch.equal(ds.table.view(torch.int32), want.view(torch.int32))
    assert len(ds) == 6 and ds.sample_shape == (4, 4, 4) and ds.latent_elems == 64
    src = ds.source()
    assert (src.rows, src.latent_dtype, src.label_dtype, src.latent_elems, src.text_emb) == (6, _lib.DTYPE_U8, _lib.DTYPE_F16, 64, 10)
    assert DeviceLatentDataset(lat.float(), torch.zeros(6, 10), device="cpu").table is None


def test_dataset_batches_are_a_shuffled_pass_with_a_short_last_batch():
    ds = DeviceLatentDataset(torch.zeros(10, 4, 2, 2, dtype=torch.float16), torch.zeros(10, 3), device="cpu")
    got = list(ds.batches(4, seed=3, epoch=0))
    assert [len(b) for b in got] == [4, 4, 2] and all(b.dtype == torch.int64 for b in got)
    assert sorted(torch.cat(got).tolist()) == list(range(10))
    again = torch.cat(list(ds.batches(4, seed=3, epoch=0)))
    assert torch.equal(again, torch.cat(got))
    assert not torch.equal(torch.cat(list(ds.batches(4, seed=3, epoch=1))), again) or not torch.equal(torch.cat(list(ds.batches(4, seed=4, epoch=0))), again)
    for bad in (dict(latents=torch.zeros(3, 4, dtype=torch.int32)), dict(text_emb=torch.zeros(3, 2, dtype=torch.float64)), dict(text_emb=torch.zeros(4, 2))):
        kw = dict(latents=torch.zeros(3, 4), text_emb=torch.zeros(3, 2))
        kw.update(bad)
        with pytest.raises((TypeError, ValueError)):
            DeviceLatentDataset(kw["latents"], kw["text_emb"], device="cpu")


# ---- the C entry: part of the ABI, and every refusal comes before any HIP call ------------------------------------------------------------------------
def _call(src=None, idx=1, batch=4, a=1.0, b=2.5, p=0.15, outs=(1, 1, 1, 1), bad=1, **src_kw):
    """Pointers are the dummy value 0x1000: a refusal must return before anything looks at them."""
    P = lambda v: C.c_void_p(0x1000) if v else None
    kw = dict(latents=0x1000, labels=0x1000, dequant_table=0x1000, rows=8, latent_dtype=_lib.DTYPE_U8, label_dtype=_lib.DTYPE_F16, latent_elems=64, text_emb=10,
              vae_scale=8.0)
    kw.update(src_kw)
    s = _lib.TldBatchSource(**kw)
    return _lib.lib().tld_train_prepare_batch(None, None if src == "null" else C.byref(s), P(idx), batch, 1, 2, 0, a, b, p, *(P(o) for o in outs), None, None, None,
                                              P(bad), None)


def test_prepare_batch_is_part_of_the_abi_and_refuses_before_any_hip_call():
    assert "tld_train_prepare_batch" in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), "tld_train_prepare_batch")
    L = _lib.lib()
    cases = [dict(src="null"), dict(idx=0), dict(latents=None), dict(labels=None), dict(bad=0),
             dict(outs=(0, 1, 1, 1)), dict(outs=(1, 0, 1, 1)), dict(outs=(1, 1, 0, 1)), dict(outs=(1, 1, 1, 0)),
             dict(batch=0), dict(batch=-3), dict(rows=0), dict(rows=-1), dict(latent_elems=0), dict(text_emb=0),
             dict(batch=(1 << 26) + 1), dict(batch=1 << 20, latent_elems=(1 << 14) + 1),
             dict(latent_dtype=_lib.DTYPE_BF16), dict(latent_dtype=7), dict(label_dtype=_lib.DTYPE_U8), dict(label_dtype=_lib.DTYPE_BF16), dict(label_dtype=-1),
             dict(dequant_table=None),
             dict(latent_dtype=_lib.DTYPE_F16, vae_scale=0.0), dict(latent_dtype=_lib.DTYPE_F32, vae_scale=float("nan")),
             dict(a=0.0), dict(a=-1.0), dict(a=float("nan")), dict(b=0.0), dict(b=float("nan")), dict(b=float("inf")),
             dict(p=-0.01), dict(p=1.01), dict(p=float("nan"))]
    for kw in cases:
        assert _call(**kw) == 1 and L.tld_last_error(), kw                       # TLD_ERR_INVALID with a reason

"""GPU: the distribution metrics (csrc/tld_metrics.hip, transformer_latent_diffusion_amd/metrics.py) against the float64
statements of tests/metrics_ref.py.

* ``tld_feat_append``: the stored rows bit for bit, for the three input types; pad columns zero; two calls equal one; bad rows counted.
* ``tld_feat_moments`` against ``np.mean`` / ``np.cov`` within 1e-12 of the largest |cov| entry (the project's figure for a fixed-order double
  reduction, tests/test_gpu_grad_guard.py); two runs bitwise equal.
* ``tld_feat_kernel_sum`` on the STORED fp32 rows, so that only the kernel's arithmetic is in the difference.  The bound is derived, not fitted
  (``metrics_ref.pair_bound``): per pair gamma (4 c |a||b| + 3 u d2_max) + 2 u |k - 1|_max with c = 1.5e-7 and u = 2^-24; a sum of N pairs divided by
  N keeps it, ``mmd2`` gets four times it.  For unit rows and sigma = 10 that is about 6e-9 per pair on values of 1e-2 and about 2.5e-8 on an MMD^2 of
  about 2e-4; a masking or diagonal mistake moves a sum by about 0.01 / n = 4e-5 at n = 257.  With TLD_METRICS_RECORD=<file> every measured error
  is appended to that file beside its bound (profiles/metrics_gpu_tests.txt is such a run).
* Shapes: (na, nb) in {(1, 1), (2, 2), (31, 33), (32, 32), (129, 130), (257, 200)} x dim in {40, 64, 768}: the smallest plans, one row short of an
  MFMA tile, exactly one, one row over a 128-row block, the pad columns, and the first multi-tile diagonal (257 rows: 3 x 3 blocks, 6 tiles run)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import metrics_ref as R
from test_clip_vision_host import vcfg
from test_gpu_parity import _dev
from transformer_latent_diffusion_amd import FeatureBank, FeatureMoments, _lib, cmmd, frechet_distance, mmd2
from transformer_latent_diffusion_amd.clip_image import ClipImageEncoder, clip_preprocess

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 2), (31, 33), (32, 32), (129, 130), (257, 200)]
DIMS = [40, 64, 768]


def _record(line):
    path = os.environ.get("TLD_METRICS_RECORD")
    print(line)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


_ROWS = {}


def _rows(n, dim, seed, normalize=True):
    """Stored bank rows [n, pitch] (host fp32, shared by the tests and never changed) of randn rows, by the append statement."""
    key = (n, dim, seed, normalize)
    if key not in _ROWS:
        x = np.random.default_rng(1000 * seed + dim).standard_normal((n, dim)).astype(np.float32)
        _ROWS[key] = R.append_ref(x, normalize)[0]
        _ROWS[key].setflags(write=False)
    return _ROWS[key]


def _up(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _ksum(a, na, b, nb, dim, gamma, same):
    """tld_feat_kernel_sum on device matrices [>= n, pitch]; workspace and result start as NaN."""
    L = _lib.lib()
    count = L.tld_feat_kernel_sum_partials(na, nb, same)
    part = torch.full((count,), float("nan"), dtype=torch.float64, device=_dev())
    out = torch.full((1,), float("nan"), dtype=torch.float64, device=_dev())
    _lib.check(L.tld_feat_kernel_sum(_ptr(a), na, _ptr(b), nb, dim, R.pitch(dim), gamma, same, _ptr(part), count, _ptr(out), _stream()), "tld_feat_kernel_sum")
    return float(out.item())


def _moments(bank_t, n, dim):
    mean = torch.full((dim,), float("nan"), dtype=torch.float64, device=_dev())
    cov = torch.full((dim, dim), float("nan"), dtype=torch.float64, device=_dev())
    _lib.check(_lib.lib().tld_feat_moments(_ptr(bank_t), n, dim, R.pitch(dim), _ptr(mean), _ptr(cov), _stream()), "tld_feat_moments")
    return mean.cpu().numpy(), cov.cpu().numpy()


# ---- 7. append --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("dim", DIMS)
def test_append_stores_the_statement_bit_for_bit(dim, dtype):
    g = torch.Generator().manual_seed(dim)
    x = (torch.randn(70, dim, generator=g) * 2).to(dtype)
    x[3] = 0
    x[9, dim - 1] = float("nan")
    x[68, 0] = float("-inf")
    want, nbad = R.append_ref(x.to(torch.float32).numpy(), True)
    one = FeatureBank(dim, 75, _dev())
    one.add(x.to(_dev()))
    two = FeatureBank(dim, 70, _dev())
    two.add(x[:13].to(_dev())).add(x[13:])                                   # (a host tensor is taken to the bank's device)
    assert len(one) == len(two) == 70 and one.bad_rows() == two.bad_rows() == nbad == 3
    got = one._data.cpu().numpy()
    assert got.shape == (75, R.pitch(dim)) and np.array_equal(got[:70].view(np.uint32), want.view(np.uint32))
    assert not got[70:].any() and not got[:, dim:].any()
    assert torch.equal(two._data, one._data[:70]) and torch.equal(one.features(), one._data[:70, :dim])
    raw = FeatureBank(dim, 70, _dev(), normalize=False)
    raw.add(x.to(_dev()))
    want_raw, nbad_raw = R.append_ref(x.to(torch.float32).numpy(), False)
    assert raw.bad_rows() == nbad_raw == 2 and np.array_equal(raw._data.cpu().numpy().view(np.uint32), want_raw.view(np.uint32))
    with pytest.raises(ValueError, match="do not fit the capacity"):
        two.add(x[:1])


# ---- 8. moments -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 33, 257])
@pytest.mark.parametrize("dim", DIMS)
def test_moments_against_numpy_and_bitwise_repeatable(dim, n):
    rows = _rows(n, dim, 1)
    dev = _up(rows)
    mean, cov = _moments(dev, n, dim)
    want_mean, want_cov = R.moments_ref(rows[:, :dim])
    scale = np.abs(want_cov).max()
    e_mean, e_cov = np.abs(mean - want_mean).max(), np.abs(cov - want_cov).max()
    _record(f"moments dim {dim} n {n}: mean error {e_mean:.2e} (bound {1e-12 * np.abs(want_mean).max():.2e}), cov error {e_cov:.2e} (bound {1e-12 * scale:.2e})")
    assert e_mean <= 1e-12 * np.abs(want_mean).max() and e_cov <= 1e-12 * scale
    assert np.array_equal(cov, cov.T)
    mean2, cov2 = _moments(dev, n, dim)
    assert np.array_equal(mean, mean2) and np.array_equal(cov, cov2)


# ---- 9. pair sums -----------------------------------------------------------------------------------------------------------------------------
def _check_sums(tag, a, b, dim, sigma):
    """The three sums and both estimators for stored rows a, b against the float64 statement, each within the derived bound."""
    na, nb, gamma = len(a), len(b), 1.0 / (2.0 * sigma * sigma)
    da, db = _up(a), _up(b)
    fa, fb = a[:, :dim], b[:, :dim]
    got, want, bound = {}, {}, {}
    for key, (x, dx, y, dy, same) in {"xx": (fa, da, fa, da, 1), "yy": (fb, db, fb, db, 1), "xy": (fa, da, fb, db, 0)}.items():
        got[key] = _ksum(dx, len(x), dy, len(y), dim, gamma, same)
        want[key] = R.kernel_sum_ref(x, y, gamma, bool(same))
        bound[key] = R.pair_bound(x, y, gamma)
        pairs = len(x) * (len(x) - 1) if same else len(x) * len(y)
        if pairs == 0:
            assert got[key] == 0.0 and want[key] == 0.0, (tag, key)             # one row against itself: the constant 0
            continue
        err = abs(got[key] - want[key]) / pairs
        _record(f"{tag} S_{key}: {got[key]:.12e} vs {want[key]:.12e}, error per pair {err:.2e} (bound {bound[key]:.2e})")
        assert math.isfinite(got[key]) and err <= bound[key], (tag, key, err, bound[key])
    for unbiased in (False, True):
        if unbiased and (na < 2 or nb < 2):
            continue                                                           # the unbiased estimator is not defined on a single row
        dx, dy = (na * (na - 1), nb * (nb - 1)) if unbiased else (na * na, nb * nb)
        est = lambda s: s["xx"] / dx + s["yy"] / dy - 2.0 * s["xy"] / (na * nb)
        err, lim = abs(est(got) - est(want)), 4.0 * max(bound.values())
        _record(f"{tag} mmd2 {'unbiased' if unbiased else 'biased'}: {est(got):.9e} vs {est(want):.9e}, error {err:.2e} (bound {lim:.2e})")
        assert abs(est(want) - R.mmd2_ref(fa, fb, sigma, unbiased)) <= 1e-15
        assert err <= lim, (tag, unbiased, err, lim)


@pytest.mark.parametrize("na,nb", SIZES)
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_sums_on_unit_rows(dim, na, nb):
    _check_sums(f"unit dim {dim} {na}x{nb} sigma 10", _rows(na, dim, 2), _rows(nb, dim, 3), dim, 10.0)


@pytest.mark.parametrize("sigma", [10.0, 30.0])
@pytest.mark.parametrize("na,nb", [(31, 33), (129, 130), (257, 200)])
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_sums_on_rows_that_are_not_normalised(dim, na, nb, sigma):
    """randn rows: d2 up to about 2 dim + a few sigma, so at sigma = 10 most terms sit at -1 and at sigma = 30 they spread over (-1, 0); the same formula
    with the actual |a||b| and d2_max."""
    _check_sums(f"randn dim {dim} {na}x{nb} sigma {sigma:g}", _rows(na, dim, 4, False), _rows(nb, dim, 5, False), dim, sigma)


def test_kernel_sum_clamps_a_negative_rounded_distance():
    """Rows that differ in their last bits: |a|^2 + |b|^2 - 2 a.b rounds to either side of 0 and max(0, .) holds it there, so no term is positive."""
    base = _rows(1, 768, 6)
    a = np.repeat(base, 130, axis=0).copy()
    a[1::2, :768] = np.nextafter(a[1::2, :768], np.float32(2.0))
    gamma = 1.0e6                                                              # makes a d2 of 1e-7 visible
    dev = _up(a)
    got = _ksum(dev, 130, dev, 130, 768, gamma, 1)
    want, bound = R.kernel_sum_ref(a[:, :768], a[:, :768], gamma, True), R.pair_bound(a[:, :768], a[:, :768], gamma)
    err = abs(got - want) / (130 * 129)
    _record(f"near-equal rows dim 768 n 130 gamma 1e6: {got:.9e} vs {want:.9e}, error per pair {err:.2e} (bound {bound:.2e})")
    assert got <= 0.0 and err <= bound


# ---- 10. ragged ends --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,na,nb", [(40, 129, 130), (64, 31, 33), (768, 257, 200)])
def test_operands_inside_larger_allocations_full_of_nan_give_the_same_bits(dim, na, nb):
    a, b = _rows(na, dim, 2), _rows(nb, dim, 3)
    p, gamma = R.pitch(dim), 0.005
    da, db = _up(a), _up(b)
    tight = (_ksum(da, na, db, nb, dim, gamma, 0), _ksum(da, na, da, na, dim, gamma, 1), _ksum(db, nb, db, nb, dim, gamma, 1))
    big = torch.full((na + nb + 300, p), float("nan"), dtype=torch.float32, device=_dev())
    va, vb = big[7:7 + na], big[7 + na + 150:7 + na + 150 + nb]                  # NaN rows before, between and after
    va.copy_(da); vb.copy_(db)
    assert va.is_contiguous() and vb.is_contiguous()
    loose = (_ksum(va, na, vb, nb, dim, gamma, 0), _ksum(va, na, va, na, dim, gamma, 1), _ksum(vb, nb, vb, nb, dim, gamma, 1))
    assert all(math.isfinite(v) for v in tight) and tight == loose
    m_tight, m_loose = _moments(da, na, dim), _moments(va, na, dim)
    assert np.array_equal(m_tight[0], m_loose[0]) and np.array_equal(m_tight[1], m_loose[1]) and np.isfinite(m_loose[1]).all()
    src = torch.full((na + 9, dim), float("nan"), dtype=torch.float32, device=_dev())
    src[4:4 + na] = da[:, :dim]
    bank = FeatureBank(dim, na, _dev(), normalize=False)
    bank.add(src[4:4 + na])
    assert bank.bad_rows() == 0 and torch.equal(bank._data, da)


# ---- 11. the diagonal -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 33, 257])
def test_same_set_diagonal_contributes_exactly_zero(n):
    dim, gamma = 40, 0.125
    same_rows = np.repeat(_rows(1, dim, 7), n, axis=0)
    ident = _up(same_rows)
    assert _ksum(ident, n, ident, n, dim, gamma, 1) == 0.0                       # identical rows: every d2 is 0, on and off the diagonal
    # rows e_0 and e_1 in turn: d2 is exactly 2 between different rows and 0 between equal ones, so only off-diagonal pairs of DIFFERENT rows appear
    two = np.zeros((n, R.pitch(dim)), dtype=np.float32)
    two[0::2, 0] = 1.0
    two[1::2, 1] = 1.0
    n0, n1 = (n + 1) // 2, n // 2
    want = 2.0 * n0 * n1 * math.expm1(-2.0 * gamma)
    dev = _up(two)
    got = _ksum(dev, n, dev, n, dim, gamma, 1)
    ulp3 = 6.0 * R.U32 * abs(want)                                               # the argument -2 gamma is exact; expm1f is within 3 ulp (OpenCL's bound for expm1)
    assert abs(got - want) <= ulp3
    assert got == _ksum(dev, n, dev, n, dim, gamma, 1)                           # bitwise repeatable
    # against a copy (same = 0) the diagonal is computed: the fp32 norm chain equals the MFMA chain bit for bit, so d2 = 0 there too
    other = dev.clone()
    full = _ksum(dev, n, other, n, dim, gamma, 0)
    assert abs(full - want) <= ulp3


def test_large_gamma_and_zero_gamma():
    a, b = _up(_rows(129, 64, 2)), _up(_rows(130, 64, 3))
    assert _ksum(a, 129, b, 130, 64, 0.0, 0) == 0.0                              # gamma 0: every k - 1 is 0
    assert _ksum(a, 129, b, 130, 64, 1e9, 0) == -129.0 * 130.0                   # every k is 0
    assert _ksum(a, 129, a, 129, 64, 1e9, 1) == -129.0 * 128.0                   # ... but for the diagonal, which stays out


# ---- 12. through Python -----------------------------------------------------------------------------------------------------------------------
def _tiny_tower(max_batch=16):
    enc = ClipImageEncoder(vcfg(14, 4, 64, layers=1, embed_dim=40), init_seed=5, max_batch=max_batch)       # width 64, one layer, grid 4, 56 px
    enc.load_state_dict(enc.state_dict())                                       # (loaded weights: no warning)
    return enc.to(_dev())


def _bank_of(enc, images, capacity=None):
    bank = FeatureBank(40, capacity or len(images), _dev())
    for i in range(0, len(images), 24):                                         # several appends
        bank.add(enc.encode_image(clip_preprocess(images[i:i + 24].to(_dev()), 56)))
    return bank


def test_banks_cmmd_and_frechet_distance_on_clip_embeddings():
    enc = _tiny_tower()
    g = torch.Generator().manual_seed(8)
    flat = torch.rand(128, 3, 56, 56, generator=g)                              # uniform pixels
    dark = torch.rand(64, 3, 56, 56, generator=g) ** 3 * torch.linspace(0.2, 1.0, 56).view(1, 1, 1, 56)      # dark, with a horizontal ramp
    half1, half2, other = _bank_of(enc, flat[:64]), _bank_of(enc, flat[64:], capacity=70), _bank_of(enc, dark)
    assert len(half1) == len(half2) == len(other) == 64 and half1.bad_rows() == half2.bad_rows() == other.bad_rows() == 0
    e1, e2, eo = (b.features().cpu().numpy() for b in (half1, half2, other))
    assert np.abs(np.sqrt((e1.astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 40 ** 0.5 * R.U32
    values = {}
    for tag, (bx, ex, by, ey) in {"null": (half1, e1, half2, e2), "different": (half1, e1, other, eo)}.items():
        lim = 4.0 * R.pair_bound(ex, ey, 1.0 / 200.0)
        for unbiased in (False, True):
            got, want = float(mmd2(bx, by, 10.0, unbiased)), R.mmd2_ref(ex, ey, 10.0, unbiased)
            _record(f"python {tag} mmd2 {'unbiased' if unbiased else 'biased'}: {got:.9e} vs {want:.9e}, error {abs(got - want):.2e} (bound {lim:.2e})")
            assert abs(got - want) <= lim
        c = cmmd(bx, by)
        assert c.device.type == "cuda" and c.dtype == torch.float64 and c.dim() == 0
        assert abs(float(c) - 1000.0 * R.mmd2_ref(ex, ey, 10.0, False)) <= 1000.0 * lim
        # the Frechet distance from the device moments against the same host formula on numpy's moments.  The device moments are within 1e-12 of the
        # largest |cov| entry (test 8); an eigenvalue moves by at most that times dim (Weyl), and |sqrt x - sqrt y| <= sqrt |x - y|
        mx, my = (FeatureMoments(len(e), *map(torch.from_numpy, R.moments_ref(e))) for e in (ex, ey))
        fd, fd_want = frechet_distance(bx, by), frechet_distance(mx, my)
        scale = max(float(mx.cov.abs().max()), float(my.cov.abs().max()))
        fd_lim = 2.0 * 40 * math.sqrt(40 * 1e-12) * scale + 1e-12 * (1.0 + fd_want)
        _record(f"python {tag} frechet: {fd:.12e} vs {fd_want:.12e}, error {abs(fd - fd_want):.2e} (bound {fd_lim:.2e})")
        assert abs(fd - fd_want) <= fd_lim
        assert abs(frechet_distance(bx.moments().cpu(), my) - fd) <= fd_lim       # banks and moment sets mix
        values[tag] = (float(c), fd)
    _record(f"python cmmd null {values['null'][0]:.6e} different {values['different'][0]:.6e}; frechet null {values['null'][1]:.6e} different {values['different'][1]:.6e}")
    assert values["different"][0] > values["null"][0] and values["different"][1] > values["null"][1]
    assert float(mmd2(half1, half1)) == 0.0                                      # a bank against itself: three equal sums
    with pytest.raises(ValueError, match="L2-normalised"):
        cmmd(half1, FeatureBank(40, 4, _dev(), normalize=False))


def test_trainer_eval_features_fills_a_bank_and_leaves_the_step_alone():
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, DenoiserConfig, TrainConfig, Trainer, VaeDecoderConfig
    dcfg = DenoiserConfig(image_size=16, noise_embed_dims=256, patch_size=2, embed_dim=256, dropout=0, n_layers=2, text_emb_size=768, n_channels=4)
    enc = _tiny_tower(max_batch=3)                                              # 8 images: chunked 3 + 3 + 2
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2, max_batch=8).to(_dev())
    tr = Trainer(dcfg, TrainConfig(batch_size=8, lr=1e-3, alpha=0.9), device=_dev(), init_seed=4, max_batch=8)
    g = torch.Generator().manual_seed(3)
    batch = lambda: (torch.randn(8, 4, 16, 16, generator=g) * 0.5, torch.rand(8, generator=g) * 0.9 + 0.05, torch.randn(8, 768, generator=g) * 0.5)
    mk = lambda x, nl, y: (x + nl.view(-1, 1, 1, 1) * torch.randn(x.shape, generator=g), nl, y, x)
    tr.forward_backward(*mk(*batch())); tr.optimizer_step()
    tr.forward_backward(*mk(*batch()), last_micro_batch=False)                  # an accumulation in progress
    state = (tr.params.clone(), tr.ema.clone(), tr.step, tr.global_step, tr._acc_n, tr.grads.clone(), None if tr._acc is None else tr._acc.clone())
    labels = torch.randn(4, 768, generator=g) * 0.5
    bank = FeatureBank(40, 16, _dev())
    lat, images = tr.eval_features(labels, vae, enc, bank, num_imgs=8, n_iter=4)
    lat2, images2 = tr.eval_generate(labels, vae, num_imgs=8, n_iter=4)
    assert torch.equal(lat, lat2) and torch.equal(images, images2) and len(bank) == 8 and bank.bad_rows() == 0
    emb = enc.encode_image(clip_preprocess((images.to(_dev()).float() * 0.5 + 0.5).clamp(0, 1), 56))
    want = R.append_ref(emb.cpu().numpy(), True)[0]
    assert np.array_equal(bank._data[:8].cpu().numpy().view(np.uint32), want.view(np.uint32))
    tr.eval_features(labels, vae, enc, bank, num_imgs=8, n_iter=4, seed=11)     # a second seed fills the rest
    assert len(bank) == 16 and not torch.equal(bank._data[8:], bank._data[:8])
    assert torch.equal(tr.params, state[0]) and torch.equal(tr.ema, state[1]) and (tr.step, tr.global_step, tr._acc_n) == state[2:5]
    assert torch.equal(tr.grads, state[5]) and (state[6] is None or torch.equal(tr._acc, state[6]))
    with pytest.raises(ValueError, match="needs a vae"):
        tr.eval_features(labels, None, enc, bank)
    with pytest.raises(ValueError, match="do not fit the capacity"):
        tr.eval_features(labels, vae, enc, bank, num_imgs=8, n_iter=4)

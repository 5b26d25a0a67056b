"""CPU: the host side of the distribution metrics -- ``frechet_distance`` against the textbook ``sqrtm`` form, the float64
statements of MMD^2 (tests/metrics_ref.py) against a direct double loop, the tile plan (csrc/tld_feat_plan.h through tests/host/feat_plan_main.cpp,
plain and under AddressSanitizer + UBSan) against the restated cut, the append statement, the refusals of the tld_feat_* entry points -- which come
before any HIP call and so need no GPU -- and the moments file."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import metrics_ref as R
from transformer_latent_diffusion_amd import FeatureBank, FeatureMoments, _lib, cmmd, frechet_distance, metrics, mmd2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SIZES = (1, 31, 32, 33, 127, 128, 129, 257)


def _moments(x):
    mean, cov = R.moments_ref(x)
    return FeatureMoments(len(x), torch.from_numpy(mean), torch.from_numpy(cov))


# ---- 1. the Frechet distance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,n", [(64, 256), (192, 768)])
def test_frechet_distance_equals_the_sqrtm_form_on_full_rank_inputs(E, n):
    x, y = R.frechet_inputs(E, n, seed=E)
    mx, my = _moments(x), _moments(y)
    want = R.frechet_sqrtm(mx.mean.numpy(), mx.cov.numpy(), my.mean.numpy(), my.cov.numpy())
    got = frechet_distance(mx, my)
    print(f"E {E} n {n}: {got:.15g} vs sqrtm {want:.15g}, relative {abs(got - want) / want:.2e}")
    assert want > 1e-3 and abs(got - want) <= 1e-10 * want
    assert abs(frechet_distance(mx, mx)) <= 1e-10 and abs(frechet_distance(my, my)) <= 1e-10
    assert abs(frechet_distance(my, mx) - got) <= 1e-10 * want


def test_frechet_distance_on_a_rank_deficient_pair_is_finite_and_real():
    x, y = R.frechet_inputs(64, 40, seed=7)
    mx, my = _moments(x), _moments(y)
    want = R.frechet_sqrtm(mx.mean.numpy(), mx.cov.numpy(), my.mean.numpy(), my.cov.numpy())
    got = frechet_distance(mx, my)
    print(f"rank-deficient: {got:.15g} vs sqrtm {want:.15g}, relative {abs(got - want) / abs(want):.2e}")
    assert isinstance(got, float) and math.isfinite(got) and abs(got - want) <= 1e-6 * abs(want)


def test_frechet_distance_refuses_other_types_and_widths():
    m8, m4 = _moments(np.random.default_rng(0).standard_normal((9, 8))), _moments(np.random.default_rng(0).standard_normal((9, 4)))
    with pytest.raises(ValueError, match="widths 8 and 4"):
        frechet_distance(m8, m4)
    with pytest.raises(TypeError):
        frechet_distance(m8, np.zeros(8))


# ---- 2. MMD^2 ---------------------------------------------------------------------------------------------------------------------------------
def _mmd2_loops(x, y, sigma, unbiased):
    g = 1.0 / (2.0 * sigma * sigma)

    def s(a, b, same):
        t = 0.0
        for i in range(len(a)):
            for j in range(len(b)):
                if same and i == j:
                    continue
                t += math.expm1(-g * float(((a[i] - b[j]) ** 2).sum()))
        return t
    n, m = len(x), len(y)
    dx, dy = (n * (n - 1), m * (m - 1)) if unbiased else (n * n, m * m)
    return s(x, x, True) / dx + s(y, y, True) / dy - 2.0 * s(x, y, False) / (n * m)


@pytest.mark.parametrize("unbiased", [False, True])
def test_mmd2_statement_equals_a_double_loop(unbiased):
    rng = np.random.default_rng(5)
    x, y = rng.standard_normal((5, 8)), rng.standard_normal((7, 8)) + 0.3
    want = _mmd2_loops(x, y, 2.0, unbiased)
    assert abs(R.mmd2_ref(x, y, 2.0, unbiased) - want) <= 1e-14 * max(1.0, abs(want))
    # the same estimator stated on k instead of k - 1: the ones cancel
    k = lambda a, b: np.exp(-R.sq_dists(a, b) / 8.0)
    kxx, kyy, kxy = k(x, x), k(y, y), k(x, y)
    if unbiased:
        direct = (kxx.sum() - np.trace(kxx)) / 20 + (kyy.sum() - np.trace(kyy)) / 42 - 2 * kxy.mean()
    else:
        direct = kxx.mean() + kyy.mean() - 2 * kxy.mean()
    assert abs(want - direct) <= 1e-13


def test_mmd2_statement_on_hand_made_cases():
    rng = np.random.default_rng(6)
    x = rng.standard_normal((6, 8))
    assert R.mmd2_ref(x, x.copy(), 3.0, False) == 0.0                      # identical sets: S_xx = S_yy = S_xy less nothing, from equal sums
    p, q = np.zeros((1, 4)), np.array([[1.0, 0.0, 0.0, 0.0]])              # two single points at distance 1
    assert R.mmd2_ref(p, q, 1.0, False) == -2.0 * math.expm1(-0.5)
    assert abs(R.mmd2_ref(p, q, 1.0, False) - (2.0 - 2.0 * math.exp(-0.5))) <= 1e-15
    y = x + 1.0
    for unbiased in (False, True):                                        # sigma -> infinity: every k - 1 -> 0
        assert abs(R.mmd2_ref(x, y, 1e9, unbiased)) <= 1e-15
    assert R.kernel_sum_ref(x, x, 0.0, True) == 0.0


# ---- 3. the tile plan -------------------------------------------------------------------------------------------------------------------------
def test_tile_plan_under_sanitizers_equals_the_restated_cut(tmp_path):
    """tests/host/feat_plan_main.cpp lays the tiles over the pair matrix and checks itself that every (i, j) is covered exactly once (same = 1:
    once through the doubling); its tile lists equal tests/metrics_ref.tile_plan and their lengths tld_feat_kernel_sum_partials.  Built twice with
    the host compiler: plain, and with -fsanitize=address,undefined (run directly, nothing preloaded)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    cases = [(na, nb, 0) for na in PLAN_SIZES for nb in PLAN_SIZES] + [(n, n, 1) for n in PLAN_SIZES]
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{na} {nb} {s}\n" for na, nb, s in cases))
    want = []
    L = _lib.lib()
    for na, nb, s in cases:
        plan = R.tile_plan(na, nb, s)
        assert len(plan) == L.tld_feat_kernel_sum_partials(na, nb, s) > 0
        cover = np.zeros((na, nb), dtype=np.int64)                          # the restatement covers every pair once, too
        for ti, tj, w in plan:
            cover[ti * R.TILE:(ti + 1) * R.TILE, tj * R.TILE:(tj + 1) * R.TILE] += 1
            if w == 2:
                cover[tj * R.TILE:(tj + 1) * R.TILE, ti * R.TILE:(ti + 1) * R.TILE] += 1
        assert (cover == 1).all(), (na, nb, s)
        want.append(f"{na} {nb} {s} {len(plan)}" + "".join(f"  {ti} {tj} {w}" for ti, tj, w in plan))
    want.append(f"tile {R.TILE} 0 failures")
    src = [os.path.join(REPO, "tests", "host", "feat_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"feat_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exe], check=True)
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
        assert r.stdout.split("\n")[:-1] == want, (tag, r.stdout[-2000:])
    assert L.tld_feat_kernel_sum_partials(0, 4, 0) == 0 and L.tld_feat_kernel_sum_partials(4, 5, 1) == 0
    assert L.tld_feat_kernel_sum_partials(30000, 30000, 1) == 235 * 236 // 2 and L.tld_feat_kernel_sum_partials(30000, 5000, 0) == 235 * 40


# ---- 4. the append statement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_append_statement(dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(9, 40, generator=g) * 3).to(dtype)
    x[2] = 0
    x[5, 7] = float("nan")
    x[6, 0] = float("inf")
    xf = x.to(torch.float32).numpy()
    out, bad = R.append_ref(xf, True)
    assert out.shape == (9, 64) and out.dtype == np.float32 and bad == 3
    assert not out[[2, 5, 6]].any() and not out[:, 40:].any()
    good = [0, 1, 3, 4, 7, 8]
    x64 = xf[good].astype(np.float64)
    direct = np.float32(x64 / np.sqrt((x64 ** 2).sum(axis=1, keepdims=True)))
    assert np.abs(out[good, :40].astype(np.float64) - direct).max() <= 2.0 ** -24          # the summation order can move the last bit, no more
    norms = np.sqrt((out[good].astype(np.float64) ** 2).sum(1))
    assert np.abs(norms - 1.0).max() <= 40 ** 0.5 * 2.0 ** -24
    raw, bad_raw = R.append_ref(xf, False)
    assert bad_raw == 2 and np.array_equal(raw[good, :40], xf[good]) and not raw[[5, 6]].any() and not raw[2].any()


# ---- 5. the refusals --------------------------------------------------------------------------------------------------------------------------
def _refused(rc, text):
    msg = _lib.lib().tld_last_error().decode()
    assert rc == 1 and text in msg, (rc, msg, text)


def test_kernel_sum_refusals_come_before_any_hip_call():
    L = _lib.lib()
    a, b = np.zeros((4, 32), dtype=np.float32), np.zeros((4, 32), dtype=np.float32)
    part, out = np.zeros(4), np.zeros(1)
    pa, pb, pp, po = (C.c_void_p(t.ctypes.data) for t in (a, b, part, out))

    def call(a=pa, na=4, b=pb, nb=4, dim=8, pitch=32, gamma=0.005, same=0, partials=pp, n_partials=4, out=po):
        return L.tld_feat_kernel_sum(a, na, b, nb, dim, pitch, gamma, same, partials, n_partials, out, None)
    _refused(call(a=None), "a is NULL")
    _refused(call(b=None), "b is NULL")
    _refused(call(partials=None), "partials is NULL")
    _refused(call(out=None), "out is NULL")
    _refused(call(dim=0), "dim 0 outside [1, 4096]")
    _refused(call(dim=4097, pitch=4128), "dim 4097 outside [1, 4096]")
    _refused(call(pitch=8), "pitch 8 is not dim rounded up to a multiple of 32 (32)")
    _refused(call(dim=33, pitch=32), "pitch 32 is not dim rounded up to a multiple of 32 (64)")
    _refused(call(na=0), "na 0, nb 4")
    _refused(call(nb=-1), "na 4, nb -1")
    _refused(call(b=pa, nb=3, same=1), "same = 1 with na 4 != nb 3")
    _refused(call(same=1), "same = 1 with a != b")
    _refused(call(gamma=-0.5), "gamma -0.5")
    _refused(call(gamma=float("nan")), "gamma nan")
    _refused(call(gamma=float("inf")), "gamma inf")
    _refused(call(na=129, nb=129, n_partials=3), "partials holds 3 doubles, the plan needs 4")
    _refused(call(b=pa, na=129, nb=129, same=1, n_partials=2), "partials holds 2 doubles, the plan needs 3")


def test_append_and_moments_refusals_come_before_any_hip_call():
    L = _lib.lib()
    bank, src, bad, mom = np.zeros((4, 32), dtype=np.float32), np.zeros((4, 8), dtype=np.float32), np.zeros(1, dtype=np.int32), np.zeros(64)
    pk, ps, pb, pm = (C.c_void_p(t.ctypes.data) for t in (bank, src, bad, mom))

    def app(bank=pk, capacity=4, used=0, dim=8, pitch=32, src=ps, dtype=0, rows=4, normalize=1, bad=pb):
        return L.tld_feat_append(bank, capacity, used, dim, pitch, src, dtype, rows, normalize, bad, None)
    _refused(app(bank=None), "bank is NULL")
    _refused(app(src=None), "src is NULL")
    _refused(app(bad=None), "bad_count is NULL")
    _refused(app(dim=5000, pitch=5024), "dim 5000 outside")
    _refused(app(pitch=16), "pitch 16 is not dim rounded up")
    _refused(app(dtype=3), "src_dtype 3")
    _refused(app(rows=0), "rows 0")
    _refused(app(used=1), "rows [1, +4) do not fit a bank of 4 rows")
    _refused(app(used=-1), "do not fit")
    _refused(app(normalize=2), "normalize 2")

    def mo(bank=pk, n=4, dim=8, pitch=32, mean=pm, cov=pm):
        return L.tld_feat_moments(bank, n, dim, pitch, mean, cov, None)
    _refused(mo(bank=None), "bank is NULL")
    _refused(mo(mean=None), "mean is NULL")
    _refused(mo(cov=None), "cov is NULL")
    _refused(mo(n=1), "n 1 (the sample covariance needs at least 2 rows)")
    _refused(mo(dim=0), "dim 0 outside")
    _refused(mo(pitch=64), "pitch 64 is not dim rounded up")


# ---- 6. the Python surface without a device -----------------------------------------------------------------------------------------------------
def test_moments_file_round_trip(tmp_path):
    x = np.random.default_rng(2).standard_normal((30, 12))
    m = _moments(x)
    path = tmp_path / "stats.npz"
    m.save(path)
    back = FeatureMoments.load(path)
    assert back.n == 30 and back.mean.dtype == torch.float64 and back.cov.dtype == torch.float64
    assert torch.equal(back.mean, m.mean) and torch.equal(back.cov, m.cov)
    assert sorted(np.load(path).files) == ["cov", "mean", "n"]                 # a plain npz
    assert frechet_distance(m, back) == frechet_distance(m, m)
    np.savez(tmp_path / "bad.npz", n=3, mean=np.zeros(4), cov=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="do not belong together"):
        FeatureMoments.load(tmp_path / "bad.npz")


def test_bank_surface_and_cmmd_refusal_without_a_device():
    bank = FeatureBank(40, 6, "cpu")
    assert len(bank) == 0 and bank.pitch == 64 and bank.features().shape == (0, 40) and metrics.feat_pitch(768) == 768
    raw = FeatureBank(40, 6, "cpu", normalize=False)
    with pytest.raises(ValueError, match="L2-normalised"):
        cmmd(bank, raw)
    with pytest.raises(ValueError, match="L2-normalised"):
        cmmd(raw, bank)
    with pytest.raises(ValueError, match="expected \\[rows, 40\\]"):
        bank.add(torch.zeros(2, 41))
    with pytest.raises(ValueError, match="do not fit the capacity 6"):
        bank.add(torch.zeros(7, 40))
    with pytest.raises(ValueError, match="fp32, fp16 or bf16"):
        bank.add(torch.zeros(2, 40, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="needs a HIP device"):           # no CPU path, and no quiet fallback
        bank.add(torch.zeros(2, 40))
    with pytest.raises(ValueError):
        FeatureBank(4097, 4, "cpu")
    with pytest.raises(ValueError, match="rows"):
        mmd2(bank, bank)

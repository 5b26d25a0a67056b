"""CPU: the host side of the stochastic sampler (tld_sample_requests_stochastic) -- the eta table of schedule.py (eta = 0 is
today's table bit for bit; the float64 table keeps the mean and the marginal standard deviation; an independently written k-diffusion-form step), its
refusals, the numpy statement of the noise's counter layout against csrc/tld_sampler_noise.h built by the host compiler (plain and under
-fsanitize=address,undefined, run as a stand-alone program), the CPU reference loop at eta = 0, the default-key rule, the refusals of the C entry that
need no device, and the sort and un-sort of the two new arrays around a stand-in library."""
import ctypes as C
import math
import os
import shutil
import subprocess
from dataclasses import asdict

import numpy as np
import pytest
import torch

import guided_ref as G
import stochastic_ref as S
from conftest import cfg_from_arr, load_golden, synth_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETAS = (0.3, 1.0, 2.0)


def _schedules():
    from transformer_latent_diffusion_amd import schedule
    return {"default 8": schedule.noise_schedule(8, 1), "exponent 2": schedule.noise_schedule(7, 2), "exponent 0.5": schedule.noise_schedule(6, 0.5),
            "truncated": schedule.truncate_levels(schedule.noise_schedule(9, 1), 0.65)[1]}


# ---- 1. the table ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_eta_zero_is_todays_table_bit_for_bit(plus):
    from transformer_latent_diffusion_amd import schedule
    for name, lv in _schedules().items():
        want = schedule.step_coefficients(lv, plus)
        for eta in (0, 0.0, -0.0, np.float32(0)):
            got = schedule.step_coefficients(lv, plus, eta=eta)
            assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.tobytes() == want.tobytes(), (name, eta)
    # and today's table is what it was: (sigma, s - t, t, s, c1, c2) rounded from float64
    lv = schedule.noise_schedule(5, 1)
    co = schedule.step_coefficients(lv, plus)
    assert co[1].tolist() == [np.float32(lv[1]), np.float32(lv[1] - lv[2]), np.float32(lv[2]), np.float32(lv[1])] + co[1, 4:].tolist()


@pytest.mark.parametrize("eta", ETAS)
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_float64_table_keeps_the_mean_and_the_marginal_deviation(plus, eta):
    """Every inner row, to 1e-12 relative, on the float64 table before the fp32 cast: (b / c) alpha_s + a / c = alpha_t (a perfect denoiser, x0 the
    clean image at every step, keeps the mean) and (b / c)^2 sigma_s^2 + e^2 = sigma_t^2 (and the marginal standard deviation)."""
    from transformer_latent_diffusion_amd import schedule
    worst = [0.0, 0.0]
    for name, lv in _schedules().items():
        tab, e = schedule.stochastic_step_coefficients_f64(lv, plus, eta)
        assert tab.dtype == np.float64 and e.dtype == np.float64 and tab.shape == (len(lv), 6) and e.shape == (len(lv),)
        assert e[-1] == 0.0 and (e[:-1] > 0).all() and tab[-1].tolist() == [lv[-1], 0.0, 0.0, 1.0, 1.0, 0.0]
        for i in range(len(lv) - 1):
            s, t = lv[i], lv[i + 1]
            sig, a, b, c = tab[i, :4]
            assert sig == s and c == s
            mean = (b / c) * (1 - s) + a / c
            var = (b / c) ** 2 * s * s + e[i] ** 2
            worst[0] = max(worst[0], abs(mean - (1 - t)) / (1 - t))
            worst[1] = max(worst[1], abs(var - t * t) / (t * t))
        tab32, e32 = schedule.step_coefficients(lv, plus, eta=eta)
        assert tab32.dtype == np.float32 and e32.dtype == np.float32 and e32.shape == (len(lv),) and e32[-1] == 0.0
        assert np.array_equal(tab32, tab.astype(np.float32)) and np.array_equal(e32, e.astype(np.float32))
        # c1, c2 are the deterministic solver's
        assert np.array_equal(tab32[:, 4:], schedule.step_coefficients(lv, plus)[:, 4:]) and np.array_equal(tab32[:, 0], schedule.step_coefficients(lv, plus)[:, 0])
    print(f"eta {eta}, {'dpm' if plus else 'ddim'}: worst relative error of the mean identity {worst[0]:.2e}, of the variance identity {worst[1]:.2e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


@pytest.mark.parametrize("eta", (0.0,) + ETAS)
@pytest.mark.parametrize("plus", [True, False], ids=["dpm", "ddim"])
def test_table_against_a_kdiffusion_form_step(plus, eta):
    """x_t = (a (c1 x0 - c2 x0_prev) + b x_s) / c + e z in float64 against sample_dpmpp_2m_sde's step ("midpoint") carried to alpha = 1 - sigma
    (stochastic_ref.kdiffusion_step): c1, c2 and the three coefficients.  eta = 0 holds today's table to the same form."""
    from transformer_latent_diffusion_amd import schedule
    rng = np.random.default_rng(5)
    worst = 0.0
    for name, lv in _schedules().items():
        if eta > 0:
            tab, e = schedule.stochastic_step_coefficients_f64(lv, plus, eta)
        else:
            tab, e = schedule.step_coefficients(lv, plus).astype(np.float64), np.zeros(len(lv))
        tol = 1e-12 if eta > 0 else 1e-6           # (today's table exists in float32 only)
        x, old = rng.standard_normal(64), None
        for i in range(len(lv) - 1):
            x0, z = rng.standard_normal(64), rng.standard_normal(64)
            _, a, b, c, c1, c2 = tab[i]
            D = c1 * x0 - c2 * (old if old is not None else 0.0)
            got = (a * D + b * x) / c + e[i] * z
            want = S.kdiffusion_step(x, x0, old if (plus and i > 0) else None, lv[i], lv[i + 1], lv[i - 1] if i > 0 else None, eta, z)
            err = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, err)
            assert err <= tol, (name, i, err)
            x, old = want, x0
    print(f"eta {eta}, {'dpm' if plus else 'ddim'}: worst relative difference from the k-diffusion-form step {worst:.2e}")


def test_refusals_of_the_table():
    from transformer_latent_diffusion_amd import schedule
    lv = schedule.noise_schedule(5, 1)
    for bad in (-0.1, float("nan"), float("inf"), -float("inf"), "x", None):
        with pytest.raises(ValueError):
            schedule.step_coefficients(lv, True, eta=bad)
        with pytest.raises(ValueError):
            schedule.step_coefficients([0.5, 0.7], True, eta=bad)           # eta is checked before the levels
    for levels in ([0.9, 0.5, 0.5, 0.2], [0.9, 0.4, 0.6, 0.2], [0.5, 0.7], [0.9, 0.5, 0.0], [1.0, 0.5, 0.2], [0.9]):
        with pytest.raises(ValueError):
            schedule.step_coefficients(levels, True, eta=0.5)
        with pytest.raises(ValueError):
            schedule.step_coefficients(levels, False, eta=0.5)
    # eta = 0 keeps today's behaviour on the same levels: a repeated level is a table (DDIM), not an error
    assert schedule.step_coefficients([0.9, 0.5, 0.5, 0.2], False, eta=0).shape == (4, 6)
    with pytest.raises(ValueError):
        schedule.stochastic_step_coefficients_f64(lv, True, 0.0)


# ---- 2. the counter layout --------------------------------------------------------------------------------------------------------------------------------
def test_numpy_counter_layout_equals_the_header_under_the_host_compiler_plain_and_sanitized(tmp_path):
    """tests/host/sampler_noise_main.cpp prints, per quad, the Philox words of csrc/tld_sampler_noise.h and the two fp32 uniforms the normals are
    made of; every bit equals stochastic_ref's.  Built twice with the host compiler: plain, and with -fsanitize=address,undefined (run directly,
    nothing preloaded, nothing loaded into Python)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    src = [os.path.join(REPO, "tests", "host", "sampler_noise_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    cases = [(0x1234, 0, 0, 1200), (0xFEDCBA9876543210, 7, 1021, 800), ((5 << 32) | 11, 63, (1 << 32) - 300, 300)]
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"sampler_noise_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exe], check=True)
        for key, step, first, n in cases:
            r = subprocess.run([exe, hex(key), str(step), str(first), str(n)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
            rows = [l.split() for l in r.stdout.split("\n") if l]
            assert len(rows) == n and [int(x[0]) for x in rows] == list(range(first, first + n))
            got = np.array([[int(v, 16) for v in x[1:13]] for x in rows], dtype=np.uint32)
            words = S.noise_words(key, step, 4 * n, first_quad=first)
            assert np.array_equal(got[:, :4], words), (tag, key, step)
            assert np.array_equal(got[:, 4:8], S.P.uniform24_open(words).view(np.uint32)), (tag, "uniform24_open")
            assert np.array_equal(got[:, 8:12], S.P.uniform24_open_complement(words).view(np.uint32)), (tag, "uniform24_open_complement")
    # the layout itself: quad in word 0, the forward in word 1, the tag in word 2, the key's halves as the Philox key
    w = S.noise_words(0xAABBCCDD11223344, 9, 4, first_quad=17)
    assert np.array_equal(w[0], S.P.philox4x32_10(np.array([17, 9, 0x534E5A31, 0], dtype=np.uint32), np.array([0x11223344, 0xAABBCCDD], dtype=np.uint32)))
    # distinct (key, step) pairs give distinct words
    a, b, c = S.noise_words(3, 0, 64), S.noise_words(3, 1, 64), S.noise_words(3 | (1 << 32), 0, 64)
    assert not (a == b).all(axis=1).any() and not (a == c).all(axis=1).any()
    hdr = open(os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc", "tld_sampler_noise.h")).read()
    assert "hip" not in hdr.replace("HIP in this file", "").lower().replace("__hipcc__", ""), "the header is to stay free of HIP"


def test_reference_normals_are_standard():
    z = S.noise_f64(77, 3, 1 << 16)
    assert abs(z.mean()) < 4 / 256 and abs(z.var() - 1) < 0.03 and np.abs(z).max() < 5.9


# ---- 3. the reference loop ------------------------------------------------------------------------------------------------------------------------------
def _tiny_ref():
    from oracle.torch_ref import TorchRefDenoiser
    g = load_golden("g1_tiny32_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    return cfg, TorchRefDenoiser(asdict(cfg), synth_weights(cfg, g["weight_seed"], g["weight_checksum"]))


def test_reference_loop_at_eta_zero_is_the_guided_reference_and_eta_moves_it():
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    gen = torch.Generator().manual_seed(91)
    B = 3
    eps, z0 = torch.randn(B, 4, 32, 32, generator=gen), torch.randn(B, 4, 32, 32, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    neg = [None, torch.randn(768, generator=gen) * 0.5, None]
    mask = torch.ones(B, 1, 32, 32)
    mask[2, :, 4:20, 8:30] = 0
    n_iter, strength, plus = [4, 3, 5], [None, None, 0.65], [True, False, True]
    levels, mix = [], []
    for b in range(B):
        lv = schedule.noise_schedule(n_iter[b], 1)
        k = 0
        if strength[b] is not None:
            k, lv = schedule.truncate_levels(lv, strength[b])
        levels.append(lv)
        mix.append(float(np.float32(lv[0])) if k > 0 else 1.0)
    g = [[3.0] * len(levels[0]), [4.5, 1.0, 4.5], [2.0] * len(levels[2])]
    z = [[torch.randn(4, 32, 32, generator=gen) for _ in lv[:-1]] for lv in levels]
    args = (ref, eps, z0, mask, labels, neg, levels, mix, g, plus)
    want = G.sample_requests(*args, 0.1, 0.1, trace=True)
    got = S.sample_requests(*args, [0.0] * B, z, 0.1, 0.1, trace=True)
    for a, w in zip(got, want):
        assert torch.equal(a, w), "eta = 0 differs from guided_ref"
    # eta on request 0 only: the others keep their bits; request 0 moves from its first state on, its first prediction does not
    one = S.sample_requests(*args, [1.0, 0.0, 0.0], z, 0.1, 0.1, trace=True)
    assert torch.equal(one[0][1:], want[0][1:]) and not torch.equal(one[0][0], want[0][0])
    assert torch.equal(one[1][0, 0], want[1][0, 0]) and not torch.equal(one[2][0, 0], want[2][0, 0])
    # with a mask the noise is added before the blend: the kept region of request 2 rides the forward process of eps whatever eta is
    two = S.sample_requests(*args, [0.0, 0.0, 2.0], z, 0.1, 0.1, trace=True)
    keep = (mask[2] == 0).expand(4, 32, 32)
    assert torch.equal(two[2][:, 2][:, keep], want[2][:, 2][:, keep]) and not torch.equal(two[2][0, 2], want[2][0, 2])
    assert torch.equal(two[0][2][keep], want[0][2][keep])


# ---- 4. keys and the Python surface -------------------------------------------------------------------------------------------------------------------
class _FakeLib:
    """Stands in for libtld_hip.so: records what tld_sample_requests_stochastic receives and writes into out_latent[k] the record's key."""

    def __init__(self, img):
        self.img, self.calls = img, []

    def tld_sample_requests_stochastic(self, h, eps, z0, m, lab, neg, recs, table, guid, ecoef, keys, n_max, sharp, bright, out, B, tx0, txt, stream):
        recs = [(r.n_levels, r.class_guidance, r.start_mix, r.has_negative) for r in recs]
        assert all(recs[k][0] >= recs[k + 1][0] for k in range(B - 1)), "records not ordered by non-increasing n_levels"
        e = np.ctypeslib.as_array(ecoef, shape=(B, n_max)).copy()
        k64 = np.ctypeslib.as_array(keys, shape=(B,)).copy()
        g = None if not guid else np.ctypeslib.as_array(guid, shape=(B, n_max)).copy()
        tab = np.ctypeslib.as_array(table, shape=(B, n_max, 6)).copy()
        self.calls.append(dict(recs=recs, e=e, keys=k64, g=g, tab=tab, n_max=n_max, B=B, entry="stochastic"))
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(B, self.img))
        for k in range(B):
            o[k] = float(int(k64[k]) & 0xFFFF) + recs[k][0] * 0.001
        return 0

    def tld_sample_requests(self, *a):
        self.calls.append(dict(entry="plain"))
        return 0

    def tld_sample_requests_guided(self, *a):
        self.calls.append(dict(entry="guided"))
        return 0

    def tld_sample(self, *a):
        self.calls.append(dict(entry="uniform"))
        return 0

    def tld_sample_from(self, *a):
        self.calls.append(dict(entry="uniform_from"))
        return 0


def _fake_denoiser(monkeypatch):
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, _lib
    m = Denoiser(**asdict(DenoiserConfig(n_channels=4)))
    fake = _FakeLib(4 * 16 * 16)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(m, "_resolve_device", lambda t=None: torch.device("cpu"))
    monkeypatch.setattr(m, "_ensure_engine", lambda n, dev: None)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    return m, fake


def test_default_key_rule_and_the_tables_travel_sorted(monkeypatch):
    from transformer_latent_diffusion_amd import DiffusionGenerator, schedule
    assert schedule.noise_key(11) == 11 and schedule.noise_key(11, 3) == 11 | (3 << 32) and schedule.noise_key(-1, 1) == 0xFFFFFFFF | (1 << 32)
    assert schedule.noise_key((7 << 32) | 5, 2) == 5 | (2 << 32)
    m, fake = _fake_denoiser(monkeypatch)
    gen = DiffusionGenerator(m, None, torch.device("cpu"), torch.float32)
    lab = torch.zeros(3, 768)
    # one batch seed: image b is the b-th image of the draw
    gen.generate_latents(lab, n_iter=4, num_imgs=3, class_guidance=3.0, seed=21, img_size=16, eta=1.0)
    c = fake.calls[-1]
    assert c["entry"] == "stochastic" and c["keys"].tolist() == [21, 21 | (1 << 32), 21 | (2 << 32)] and c["g"] is None
    co, e = schedule.step_coefficients(schedule.noise_schedule(4, 1), True, eta=1.0)
    assert all(np.array_equal(c["tab"][k], co) and np.array_equal(c["e"][k], e) for k in range(3)) and [r[1] for r in c["recs"]] == [3.0] * 3
    # one int seed per request: each is image 0 of its own draw -- the one-image call with that seed has the same key
    out = gen.generate_latents_requests(lab, n_iter=[4, 6, 5], class_guidance=3.0, seeds=[5, 6, 7], img_size=16, eta=[1.0, 0.0, 0.5], use_ddpm_plus=[True, True, False])
    c = fake.calls[-1]
    assert c["entry"] == "stochastic" and [r[0] for r in c["recs"]] == [6, 5, 4] and c["keys"].tolist() == [6, 7, 5]          # engine order
    assert [float(out[b, 0, 0, 0]) for b in range(3)] == [np.float32(5 + 0.004), np.float32(6 + 0.006), np.float32(7 + 0.005)]     # and back
    assert not c["e"][0].any()                                                                # eta 0 inside a stochastic call: zeros, today's table
    assert np.array_equal(c["tab"][0], schedule.step_coefficients(schedule.noise_schedule(6, 1), True))
    co5, e5 = schedule.step_coefficients(schedule.noise_schedule(5, 1), False, eta=0.5)
    assert np.array_equal(c["tab"][1, :5], co5) and np.array_equal(c["e"][1, :5], e5) and not c["e"][1, 5:].any()
    gen.generate_latents(lab[:1], n_iter=4, num_imgs=1, class_guidance=3.0, seed=5, img_size=16, eta=1.0)
    assert fake.calls[-1]["keys"].tolist() == [5]
    # noise_seeds win; a tensor of start noise needs them
    x = torch.zeros(3, 4, 16, 16)
    gen.generate_latents(lab, n_iter=4, num_imgs=3, class_guidance=3.0, seeds=x, img_size=16, eta=1.0, noise_seeds=[9, 8, (1 << 64) - 1])
    assert fake.calls[-1]["keys"].tolist() == [9, 8, (1 << 64) - 1]
    n = len(fake.calls)
    for call in (lambda: gen.generate_latents(lab, n_iter=4, num_imgs=3, seeds=x, img_size=16, eta=1.0),
                 lambda: gen.generate_latents_requests(lab, n_iter=4, seeds=x, img_size=16, eta=[0.0, 0.0, 0.1]),
                 lambda: gen.generate_latents_from(x, lab, seeds=x, eta=0.5),
                 lambda: gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, eta=-1.0),
                 lambda: gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, eta=float("nan")),
                 lambda: gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, eta=[1.0, 1.0]),
                 lambda: gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, eta=1.0, noise_seeds=[1, 2])):
        with pytest.raises(ValueError):
            call()
    assert len(fake.calls) == n, "a refused call reached the engine"
    # eta = 0 is today's call: the uniform entries, and the plain requests entry
    gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, eta=0.0)
    gen.generate_latents_from(x, lab, seed=1, eta=0)
    gen.generate_latents_requests(lab, n_iter=[4, 5, 6], seed=1, img_size=16, eta=[0.0, 0, 0.0])
    assert [c["entry"] for c in fake.calls[n:]] == ["uniform", "uniform_from", "plain"]
    # image-to-image routes with its truncated schedule and start mix
    gen.generate_latents_from(x, lab, strength=0.65, n_iter=8, seed=3, eta=1.0)
    c = fake.calls[-1]
    k, lv = schedule.truncate_levels(schedule.noise_schedule(8, 1), 0.65)
    co, e = schedule.step_coefficients(lv, True, eta=1.0)
    assert c["entry"] == "stochastic" and np.array_equal(c["tab"][2], co) and np.array_equal(c["e"][2], e) and c["recs"][0][2] == np.float32(lv[0])
    # the Denoiser's own refusals
    tabs = [co] * 3
    for kw in (dict(noise_coeffs=[e] * 3), dict(noise_keys=[1, 2, 3]), dict(noise_coeffs=[e] * 2, noise_keys=[1, 2, 3]), dict(noise_coeffs=[e] * 3, noise_keys=[1, 2]),
               dict(noise_coeffs=[e, e[:-1], e], noise_keys=[1, 2, 3]), dict(noise_coeffs=[e, -e, e], noise_keys=[1, 2, 3]),
               dict(noise_coeffs=[e, np.full_like(e, 0.1), e], noise_keys=[1, 2, 3]), dict(noise_coeffs=[e, np.full_like(e, np.nan), e], noise_keys=[1, 2, 3]),
               dict(noise_coeffs=[e] * 3, noise_keys=[1, -2, 3]), dict(noise_coeffs=[e] * 3, noise_keys=[1, 1 << 64, 3])):
        with pytest.raises(ValueError):
            m.sample_latents_requests(x, lab, tabs, [3.0] * 3, **kw)


def test_pipeline_and_batcher_pass_eta_through():
    from transformer_latent_diffusion_amd import RequestBatcher

    class Pipe:
        def __init__(self):
            self.calls = []

        def generate_images_from_texts(self, prompts, **kw):
            self.calls.append(kw)
            return list(prompts)

    pipe = Pipe()
    rb = RequestBatcher(pipe, max_batch=4, mixed=True)
    t = [rb.submit("a", 6, 1, 15, eta=1.0), rb.submit("b", 3, 2, 15)]
    assert rb.flush() == {t[0]: "a", t[1]: "b"} and pipe.calls[0]["eta"] == [1.0, 0.0]
    rb.submit("c", 3, 2, 15)
    rb.flush()
    assert "eta" not in pipe.calls[1]                                   # no eta in the call: the keyword is not passed
    with pytest.raises(ValueError):
        rb.submit("d", eta=-1)
    # the grouped batcher groups by eta as it does by guidance
    pipe = Pipe()
    rb = RequestBatcher(pipe, max_batch=4)
    t = [rb.submit("a", 6, 1, 15, eta=1.0), rb.submit("b", 6, 2, 15), rb.submit("c", 6, 3, 15, eta=1.0), rb.submit("d", 6, 4, 15, eta=0.5)]
    plan = rb.plan()
    assert sorted(len(c[2]) for c in plan) == [1, 1, 2] and all(len(c) == 3 for c in plan)
    assert rb.flush() == dict(zip(t, "abcd"))
    assert sorted((c.get("eta", 0.0), len(c["seeds"])) for c in pipe.calls) == [(0.0, 1), (0.5, 1), (1.0, 2)]
    assert not rb._etas


# ---- 5. the C entry's refusals that need no device ----------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_stochastic_calls_before_any_hip_call():
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    Rq = _lib.TldSampleRequest
    tab = np.zeros((2, 5, 6), dtype=np.float32)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    keys = np.array([1, 2], dtype=np.uint64)

    def call(r0, r1, e, k=keys, g=None, n_max=5):
        recs = (Rq * 2)(r0, r1)
        kp = None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64))
        return L.tld_sample_requests_stochastic(None, None, None, None, None, None, recs, fp(tab), fp(g), fp(e), kp, n_max, 0.0, 0.0, None, 2, None, None, None)

    ok = np.full((2, 5), 0.25, dtype=np.float32)
    ok[:, 4] = 0
    r5 = Rq(5, 3.0, 1.0, 0)
    assert call(r5, r5, ok, k=None) == 1 and b"noise_keys" in L.tld_last_error()
    assert call(r5, r5, None) == 1 and b"noise_coeff" in L.tld_last_error()
    for v, word in ((-0.5, b">= 0"), (np.nan, b">= 0"), (np.inf, b">= 0")):
        bad = ok.copy(); bad[1, 2] = v
        assert call(r5, r5, bad) == 1 and b"request 1" in L.tld_last_error() and b"forward 2" in L.tld_last_error() and word in L.tld_last_error()
    bad = ok.copy(); bad[0, 4] = 0.25
    assert call(r5, r5, bad) == 1 and b"request 0" in L.tld_last_error() and b"final forward 4" in L.tld_last_error()
    short = ok.copy(); short[1, 2] = 0.25                               # request 1 has 3 levels: its final forward is 2
    assert call(r5, Rq(3, 3.0, 1.0, 0), short) == 1 and b"request 1" in L.tld_last_error() and b"final forward 2" in L.tld_last_error()
    first3 = ok.copy(); first3[0, 2] = 0
    assert call(Rq(3, 3.0, 1.0, 0), r5, first3) == 1 and b"non-increasing" in L.tld_last_error()
    assert call(r5, Rq(1, 3.0, 1.0, 0), ok) == 1 and b"two noise levels" in L.tld_last_error()
    assert call(Rq(5, float("nan"), 1.0, 0), r5, ok) == 1 and b"class_guidance" in L.tld_last_error()       # guidance NULL: the records' scales count
    gbad = np.full((2, 5), 3.0, dtype=np.float32); gbad[0, 1] = np.inf
    assert call(r5, r5, ok, g=gbad) == 1 and b"forward 1" in L.tld_last_error()
    past = ok.copy(); past[1, 2] = 0; past[1, 3:] = np.nan             # entries past n_levels are ignored
    assert call(r5, Rq(3, 3.0, 1.0, 0), past) == 1 and b"null" in L.tld_last_error()                         # valid: the NULL engine is next
    assert call(r5, r5, ok, g=np.full((2, 5), 3.0, dtype=np.float32)) == 1 and b"null" in L.tld_last_error()
    assert L.tld_debug_sampler_noise(None, None, 1, 4, None, None) == 1 and b"null" in L.tld_last_error()

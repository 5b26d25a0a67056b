"""CPU: the host side of the shaped guidance update (tld_sample_requests_shaped) -- guidance rescale and adaptive projected
guidance.  The algebraic statement (five sums, two fp32 weights, one fma) against the direct float64 one (project, clip, torch.std rescale); its two
defining properties in float64; csrc/tld_guidance_shape.h built by the host compiler with -ffp-contract=off, plain and under
-fsanitize=address,undefined, run as a stand-alone program, bit for bit against the numpy statement; neutral detection; the ValueErrors; the C
entries' refusals that need no device; the key and group rule of the batcher; the reference loop with neutral rows; and the way the table travels
around a stand-in library.  Every test prints the figures it asserts."""
import ctypes as C
import os
import shutil
import struct
import subprocess
from dataclasses import asdict

import numpy as np
import pytest
import torch

import shaped_ref as R
import stochastic_ref as S
from conftest import cfg_from_arr, load_golden, synth_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMGS = (64, 576, 4096)
# (eta_par, norm_r, beta, phi), g: rescale alone at phi = 1 and 0.7, APG with the clip active (r = 2.5) and inactive (r = 1e4: the test checks
# which), momentum on, and everything together
SETS = [((1.0, 0.0, 0.0, 1.0), 6.0), ((1.0, 0.0, 0.0, 0.7), 3.0), ((0.0, 2.5, 0.0, 0.0), 6.0), ((0.5, 1e4, -0.5, 0.0), 4.5),
        ((0.0, 2.5, -0.75, 1.0), 6.0), ((0.25, 0.0, 0.5, 0.4), 7.5)]


def _inputs(n, seed):
    """The inputs of the issue's check: c with mean 0.3, u = 0.8 c + 0.4 noise; and a momentum buffer like an earlier update."""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal(n) + 0.3).astype(np.float32)
    u = (np.float32(0.8) * c + np.float32(0.4) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    m = (np.float32(0.2) * c + np.float32(0.4) * rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    return c, u, m


# ---- 1. the algebraic statement is the direct one -------------------------------------------------------------------------------------------------------
def test_algebraic_statement_equals_the_direct_float64_statement():
    """max |x0 - direct| <= 2e-7 max |x0|: fp32 P and Q carry at most 2^-24 relative each, the rounded product and the fma two more half-ulps, and
    the algebra itself is exact."""
    worst, clipped = 0.0, set()
    for n in IMGS:
        c, u, m = _inputs(n, 100 + n)
        for row, g in SETS:
            st = R.statement(c, u, m, g, row)
            want = R.direct_f64(c, st["dbar"], g, row)
            err = float(np.abs(st["x0"].astype(np.float64) - want).max() / np.abs(want).max())
            worst = max(worst, err)
            if row[1] > 0:
                clipped.add(row[1] < np.sqrt(st["sums"][4]))
            assert err <= 2e-7, (n, row, g, err)
    assert clipped == {True, False}, "the sets are to cover the clip active and inactive"
    print(f"algebraic statement against the direct float64 one: worst max-relative difference {worst:.2e} over {len(IMGS)} sizes x {len(SETS)} sets")


def test_the_two_defining_properties_in_float64():
    """phi = 1: std(x0) = std(c).  eta_par = 0 without clip and momentum: <x0 - c, c> = 0.  On the float64 weights, scale-relative 1e-12."""
    worst = [0.0, 0.0]
    for n in IMGS:
        c, u, m = _inputs(n, 200 + n)
        c64 = c.astype(np.float64)
        for row, g in (((1.0, 0.0, 0.0, 1.0), 6.0), ((0.3, 3.0, -0.5, 1.0), 4.0), ((0.0, 0.0, 0.0, 1.0), 7.0)):
            db = R.dbar_f32(c, u, m, row[2]).astype(np.float64)
            P, Q = R.finalize(R.sums_f64(c, db), n, g, row, round32=False)
            x0 = P * c64 + Q * db
            worst[0] = max(worst[0], abs(x0.std() - c64.std()) / c64.std())
        for g in (6.0, 1.5, 0.0):
            db = R.dbar_f32(c, u, m, 0.0).astype(np.float64)
            P, Q = R.finalize(R.sums_f64(c, db), n, g, (0.0, 0.0, 0.0, 0.0), round32=False)
            x0 = P * c64 + Q * db
            assert np.abs(x0 - c64).max() > 0.0 or g == 1.0
            worst[1] = max(worst[1], abs(np.dot(x0 - c64, c64)) / (np.linalg.norm(x0 - c64) * np.linalg.norm(c64)))
    print(f"float64 properties: |std(x0) - std(c)| / std(c) {worst[0]:.2e}; |<x0 - c, c>| / (|x0 - c| |c|) {worst[1]:.2e}")
    assert worst[0] <= 1e-12 and worst[1] <= 1e-12


def test_fma_helper_rounds_once():
    """shaped_ref.fma_f32 against exact rational arithmetic on values chosen to sit on float32 ties after the float64 sum."""
    from fractions import Fraction
    rng = np.random.default_rng(7)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-9, 3, 4000)).astype(np.float32)
    # ties: a b + c lands within a float64 ulp of the midpoint of two float32 values
    a[:3] = np.float32(1 + 2 ** -23); b[:3] = np.float32(1 + 2 ** -23)
    c[:3] = [np.float32(2 ** -24), np.float32(-2 ** -24), np.float32(2 ** -25)]
    got = R.fma_f32(a, b, c)
    for k in range(a.size):
        exact = Fraction(float(a[k])) * Fraction(float(b[k])) + Fraction(float(c[k]))
        lo = np.float32(float(exact))                                   # (float(Fraction) rounds once to float64; settle the float32 neighbours exactly)
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert got[k] == best, (k, a[k], b[k], c[k], got[k], best)


# ---- 2. the header under the host compiler --------------------------------------------------------------------------------------------------------------
def _hex32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(np.float32(v))))[0]


def _hex64(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def test_header_finalisation_equals_the_numpy_statement_under_the_host_compiler_plain_and_sanitized(tmp_path):
    """tests/host/guidance_shape_main.cpp runs guidance_shape_finalize of csrc/tld_guidance_shape.h on sums handed over as bit patterns; P and Q equal
    shaped_ref.finalize's bit for bit.  Built twice with the host compiler and -ffp-contract=off: plain, and with -fsanitize=address,undefined (run
    directly, nothing preloaded, nothing loaded into Python)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    src = [os.path.join(REPO, "tests", "host", "guidance_shape_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    cases = []
    for n in IMGS + (6, 2304):
        c, u, m = _inputs(n, 300 + n)
        for row, g in SETS + [((1.0, 0.0, 0.0, 0.0), 6.0), ((0.0, 1e-3, 0.0, 1.0), 1.0), ((2.0, 0.0, 0.99, 0.5), -2.0)]:
            cases.append((n, g, row, R.sums_f64(c, R.dbar_f32(c, u, m, row[2]))))
    # degenerate sums: c = 0 (no projection, no rescale), u = c (no update), one element (no variance)
    cases += [(8, 6.0, (0.0, 1.0, 0.0, 1.0), [0.0, 3.0, 0.0, 0.0, 2.0]), (8, 6.0, (0.5, 1.0, 0.0, 1.0), [2.0, 0.0, 1.5, 0.0, 0.0]),
              (1, 6.0, (0.0, 0.5, 0.0, 1.0), [2.0, 1.0, 4.0, 2.0, 1.0])]
    want = [R.finalize(sums, n, g, row) for n, g, row, sums in cases]
    args = []
    for n, g, row, sums in cases:
        args += [str(n), _hex32(g)] + [_hex32(v) for v in row] + [_hex64(v) for v in sums]
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"guidance_shape_main_{tag}")
        subprocess.run([cxx, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", *flags, *src, "-o", exe], check=True)
        r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
        rows = [l.split() for l in r.stdout.split("\n") if l]
        assert len(rows) == len(cases)
        for (n, g, row, sums), (P, Q), got in zip(cases, want, rows):
            assert got[0] == _hex32(P) and got[1] == _hex32(Q), (tag, n, g, row, got, _hex32(P), _hex32(Q))
            assert int(got[2]) == int(R.is_neutral(row)) and got[3] == "0", (tag, row, got)
        bad = subprocess.run([exe, "4", _hex32(6.0), _hex32(-1.0), _hex32(0.0), _hex32(0.0), _hex32(0.0)] + [_hex64(1.0)] * 5, stdout=subprocess.PIPE, text=True)
        assert bad.returncode == 0 and bad.stdout.split()[3] == "1"
        assert subprocess.run([exe, "4"], stderr=subprocess.PIPE).returncode == 2
    assert all(np.isfinite(P) and np.isfinite(Q) for P, Q in want)
    assert want[-3] == (np.float32(1.0), np.float32(5.0 / np.sqrt(2.0)))              # c = 0: p = 0, no rescale; the clip alone
    assert want[-2] == (np.float32(1.0), np.float32(5.0))                             # no update: A = 1, B = g - 1 on dbar = 0; vx = vc
    print(f"header finalisation: {len(cases)} cases bit-equal to the numpy statement, plain and under address + undefined sanitizers")
    hdr = open(os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc", "tld_guidance_shape.h")).read()
    assert "hip" not in hdr.replace("HIP in this file", "").lower().replace("__hipcc__", ""), "the header is to stay free of HIP"


# ---- 3. neutral rows and the ValueErrors ----------------------------------------------------------------------------------------------------------------
def test_neutral_detection_and_value_errors():
    from transformer_latent_diffusion_amd import schedule
    assert schedule.check_guidance_shape() == schedule.GUIDANCE_SHAPE_NEUTRAL == (1.0, 0.0, 0.0, 0.0)
    assert schedule.guidance_shape_neutral(schedule.check_guidance_shape(0, 1, 0, 0)) and schedule.guidance_shape_neutral((1, 0, -0.0, 0))
    for kw in (dict(guidance_rescale=0.5), dict(apg_eta=0.0), dict(apg_norm=2.5), dict(apg_momentum=-0.5), dict(apg_eta=1.0 + 2.0 ** -23)):
        assert not schedule.guidance_shape_neutral(schedule.check_guidance_shape(**kw)), kw
    # the row is (eta_par, norm_r, beta, phi), in float32 values
    assert schedule.check_guidance_shape(0.7, 0.25, 2.5, -0.5) == (0.25, 2.5, -0.5, float(np.float32(0.7)))
    assert schedule.check_guidance_shape(guidance_rescale=1, apg_eta=0, apg_norm=1e30, apg_momentum=0.999) == (0.0, float(np.float32(1e30)), float(np.float32(0.999)), 1.0)
    for kw in (dict(guidance_rescale=-0.1), dict(guidance_rescale=1.0001), dict(guidance_rescale=float("nan")), dict(apg_eta=-1e-3), dict(apg_eta=float("inf")),
               dict(apg_norm=-1.0), dict(apg_norm=float("nan")), dict(apg_norm=1e39), dict(apg_momentum=1.0), dict(apg_momentum=-1.0), dict(apg_momentum=float("nan")),
               dict(apg_momentum=1.0 - 1e-9), dict(apg_eta="x"), dict(guidance_rescale=None)):
        with pytest.raises(ValueError):
            schedule.check_guidance_shape(**kw)
    # per-request rows: None where every request is neutral
    assert schedule.guidance_shape_rows(3) is None and schedule.guidance_shape_rows(3, 0.0, [1, 1, 1], 0, [0, 0, 0]) is None
    rows = schedule.guidance_shape_rows(3, [0, 0.5, 0], 1.0, 0.0, [0, 0, -0.5])
    assert rows == [(1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.5), (1.0, 0.0, -0.5, 0.0)]
    with pytest.raises(ValueError):
        schedule.guidance_shape_rows(3, [0, 0.5])
    with pytest.raises(ValueError):
        schedule.guidance_shape_rows(3, 0.0, [1, 1, -1])


# ---- 4. the Python surface around a stand-in library ----------------------------------------------------------------------------------------------------
class _FakeLib:
    """Stands in for libtld_hip.so: records which entry is called and what tld_sample_requests_shaped receives."""

    def __init__(self, img):
        self.img, self.calls = img, []

    def tld_sample_requests_shaped(self, h, eps, z0, m, lab, neg, recs, table, guid, ecoef, keys, shape, n_max, sharp, bright, out, B, tx0, txt, stream):
        recs = [(r.n_levels, r.class_guidance, r.start_mix, r.has_negative) for r in recs]
        assert all(recs[k][0] >= recs[k + 1][0] for k in range(B - 1)), "records not ordered by non-increasing n_levels"
        self.calls.append(dict(entry="shaped", recs=recs, shape=np.ctypeslib.as_array(shape, shape=(B, 4)).copy(),
                               e=None if not ecoef else np.ctypeslib.as_array(ecoef, shape=(B, n_max)).copy(),
                               keys=None if not keys else np.ctypeslib.as_array(keys, shape=(B,)).copy(),
                               g=None if not guid else np.ctypeslib.as_array(guid, shape=(B, n_max)).copy()))
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(B, self.img))
        for k in range(B):
            o[k] = recs[k][0] + 0.125 * float(self.calls[-1]["shape"][k, 3])
        return 0


for _name in ("tld_sample_requests_stochastic", "tld_sample_requests", "tld_sample_requests_guided", "tld_sample", "tld_sample_from"):
    def _entry(self, *a, _name=_name):
        self.calls.append(dict(entry=_name))
        return 0
    setattr(_FakeLib, _name, _entry)


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


def test_neutral_values_make_the_old_call_and_the_table_travels_sorted(monkeypatch):
    from transformer_latent_diffusion_amd import DiffusionGenerator
    m, fake = _fake_denoiser(monkeypatch)
    gen = DiffusionGenerator(m, None, torch.device("cpu"), torch.float32)
    lab, x = torch.zeros(3, 768), torch.zeros(3, 4, 16, 16)
    neutral = dict(guidance_rescale=0.0, apg_eta=1.0, apg_norm=0.0, apg_momentum=0.0)
    gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, **neutral)
    gen.generate_latents_from(x, lab, seed=1, **neutral)
    gen.generate_latents_requests(lab, n_iter=[4, 5, 6], seed=1, img_size=16, **neutral)
    gen.generate_latents_requests(lab, n_iter=[4, 5, 6], seed=1, img_size=16, guidance_rescale=[0, 0, 0], apg_eta=[1, 1, 1])
    gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, eta=1.0, **neutral)
    gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, guidance_interval=(0.2, 0.8), **neutral)
    assert [c["entry"] for c in fake.calls] == ["tld_sample", "tld_sample_from", "tld_sample_requests", "tld_sample_requests", "tld_sample_requests_stochastic",
                                                "tld_sample_requests_guided"]
    # a uniform call with any control set: B equal records through the new entry, no noise, no guidance table
    gen.generate_latents(lab, n_iter=4, num_imgs=3, class_guidance=6.0, seed=1, img_size=16, guidance_rescale=0.7)
    c = fake.calls[-1]
    assert c["entry"] == "shaped" and c["e"] is None and c["keys"] is None and c["g"] is None
    assert np.array_equal(c["shape"], np.tile(np.array([1, 0, 0, 0.7], np.float32), (3, 1))) and [r[1] for r in c["recs"]] == [6.0] * 3
    gen.generate_latents_from(x, lab, strength=0.65, n_iter=8, seed=3, apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5)
    assert fake.calls[-1]["entry"] == "shaped" and np.array_equal(fake.calls[-1]["shape"], np.tile(np.array([0, 2.5, -0.5, 0], np.float32), (3, 1)))
    # per request, with eta and an interval: engine order there, the caller's order back
    out = gen.generate_latents_requests(lab, n_iter=[4, 6, 5], seeds=[5, 6, 7], img_size=16, guidance_rescale=[0.5, 0.0, 1.0], apg_eta=[1.0, 1.0, 0.25],
                                        apg_momentum=[0.0, 0.0, -0.5], eta=[0.0, 1.0, 0.0], guidance_interval=[None, (0.2, 0.8), None])
    c = fake.calls[-1]
    assert c["entry"] == "shaped" and [r[0] for r in c["recs"]] == [6, 5, 4] and c["keys"].tolist() == [6, 7, 5] and c["g"] is not None and c["e"][0].any()
    assert np.array_equal(c["shape"], np.array([[1, 0, 0, 0], [0.25, 0, -0.5, 1], [1, 0, 0, 0.5]], np.float32))
    assert [float(out[b, 0, 0, 0]) for b in range(3)] == [4 + 0.0625, 6.0, 5 + 0.125]
    # refusals reach no entry
    n = len(fake.calls)
    for call in (lambda: gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, guidance_rescale=1.5),
                 lambda: gen.generate_latents(lab, n_iter=4, num_imgs=3, seed=1, img_size=16, apg_momentum=1.0),
                 lambda: gen.generate_latents_from(x, lab, seed=1, apg_norm=-1.0),
                 lambda: gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, apg_eta=[1.0, 0.5]),
                 lambda: gen.generate_latents_requests(lab, n_iter=4, seed=1, img_size=16, apg_eta=[1.0, 0.5, float("nan")]),
                 lambda: m.sample_latents_requests(x, lab, [np.zeros((4, 6), np.float32)] * 3, [3.0] * 3, shape=[(1, 0, 0, 0)] * 2),
                 lambda: m.sample_latents_requests(x, lab, [np.zeros((4, 6), np.float32)] * 3, [3.0] * 3, shape=[(1, 0, 0)] * 3),
                 lambda: m.sample_latents_requests(x, lab, [np.zeros((4, 6), np.float32)] * 3, [3.0] * 3, shape=[(1, 0, 0, 0), (1, 0, 1.0, 0), (1, 0, 0, 0)])):
        with pytest.raises(ValueError):
            call()
    assert len(fake.calls) == n, "a refused call reached the engine"
    # Denoiser.sample_latents_requests(shape=...) with neutral rows still takes the new entry: the table is the caller's choice there
    m.sample_latents_requests(x, lab, [np.zeros((4, 6), np.float32)] * 3, [3.0] * 3, shape=[(1, 0, 0, 0)] * 3)
    assert fake.calls[-1]["entry"] == "shaped"


def test_batcher_key_and_group_rule_and_the_pipeline_keywords():
    from transformer_latent_diffusion_amd import RequestBatcher

    class Pipe:
        def __init__(self):
            self.calls = []

        def generate_images_from_texts(self, prompts, **kw):
            self.calls.append(kw)
            return list(prompts)

    pipe = Pipe()
    rb = RequestBatcher(pipe, max_batch=4, mixed=True)
    t = [rb.submit("a", 6, 1, 15, guidance_rescale=0.7), rb.submit("b", 3, 2, 15), rb.submit("c", 3, 2, 15, apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5)]
    assert rb.flush() == dict(zip(t, "abc"))
    kw = pipe.calls[0]
    assert kw["guidance_rescale"] == [float(np.float32(0.7)), 0.0, 0.0] and kw["apg_eta"] == [1.0, 1.0, 0.0] and kw["apg_norm"] == [0.0, 0.0, 2.5]
    assert kw["apg_momentum"] == [0.0, 0.0, -0.5]
    rb.submit("d", 3, 2, 15)
    rb.flush()
    assert not {"guidance_rescale", "apg_eta", "apg_norm", "apg_momentum"} & set(pipe.calls[1])          # no control in the call: no keyword is passed
    for bad in (dict(guidance_rescale=2), dict(apg_eta=-1), dict(apg_norm=-1), dict(apg_momentum=1)):
        with pytest.raises(ValueError):
            rb.submit("e", **bad)
    assert rb.pending() == 0
    # the grouped batcher groups by the four values as it does by guidance and eta: equal rows share a call, anything else does not
    pipe = Pipe()
    rb = RequestBatcher(pipe, max_batch=4)
    t = [rb.submit("a", 6, 1, 15, guidance_rescale=0.7), rb.submit("b", 6, 2, 15), rb.submit("c", 6, 3, 15, guidance_rescale=0.7),
         rb.submit("d", 6, 4, 15, guidance_rescale=0.7, apg_eta=0.5), rb.submit("e", 6, 5, 15, guidance_rescale=0.0, apg_eta=1.0),
         rb.submit("f", 6, 6, 15, guidance_rescale=0.7, eta=1.0)]
    plan = rb.plan()
    assert sorted(len(c[2]) for c in plan) == [1, 1, 2, 2] and all(len(c) == 3 for c in plan)
    assert sorted(sorted(p for _, p, _ in c[2]) for c in plan) == [["a", "c"], ["b", "e"], ["d"], ["f"]]
    assert rb.flush() == dict(zip(t, "abcdef"))
    seen = sorted((c.get("guidance_rescale", [0.0])[0], c.get("apg_eta", [1.0])[0], c.get("eta", 0.0), len(c["seeds"])) for c in pipe.calls)
    r = float(np.float32(0.7))
    assert seen == [(0.0, 1.0, 0.0, 2), (r, 0.5, 0.0, 1), (r, 1.0, 0.0, 2), (r, 1.0, 1.0, 1)]
    assert all(len(c["guidance_rescale"]) == len(c["seeds"]) for c in pipe.calls if "guidance_rescale" in c)
    assert not rb._shapes and not rb._etas


# ---- 5. the C entries' refusals that need no device -----------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_shaped_calls_before_any_hip_call():
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    Rq = _lib.TldSampleRequest
    tab = np.zeros((2, 5, 6), dtype=np.float32)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    keys = np.array([1, 2], dtype=np.uint64)
    ok_e = np.full((2, 5), 0.25, dtype=np.float32)
    ok_e[:, 4] = 0
    ok_s = np.array([[1, 0, 0, 0], [0.5, 2.5, -0.5, 1.0]], dtype=np.float32)
    r5 = Rq(5, 3.0, 1.0, 0)

    def call(shape, e=ok_e, k=keys, g=None, r0=r5, r1=r5, batch=2):
        recs = (Rq * 2)(r0, r1)
        kp = None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64))
        rc = L.tld_sample_requests_shaped(None, None, None, None, None, None, recs, fp(tab), fp(g), fp(e), kp, fp(shape), 5, 0.0, 0.0, None, batch, None, None, None)
        return rc, L.tld_last_error()

    rc, msg = call(None)
    assert rc == 1 and b"shape" in msg
    for col, v, word in ((0, -0.5, b"eta_par"), (0, np.nan, b"eta_par"), (0, np.inf, b"eta_par"), (1, -1.0, b"norm_r"), (1, np.nan, b"norm_r"), (1, np.inf, b"norm_r"),
                         (2, 1.0, b"beta"), (2, -1.0, b"beta"), (2, np.nan, b"beta"), (3, -0.1, b"phi"), (3, 1.5, b"phi"), (3, np.nan, b"phi")):
        bad = ok_s.copy()
        bad[1, col] = v
        rc, msg = call(bad)
        assert rc == 1 and b"request 1" in msg and word in msg, (col, v, msg)
    rc, msg = call(ok_s, e=ok_e, k=None)
    assert rc == 1 and b"come together" in msg
    rc, msg = call(ok_s, e=None, k=keys)
    assert rc == 1 and b"come together" in msg
    rc, msg = call(ok_s, batch=0)
    assert rc == 1 and b"positive" in msg
    # the checks of the entry it generalises still run
    bad_e = ok_e.copy(); bad_e[0, 4] = 0.25
    rc, msg = call(ok_s, e=bad_e)
    assert rc == 1 and b"final forward 4" in msg
    rc, msg = call(ok_s, r1=Rq(1, 3.0, 1.0, 0))
    assert rc == 1 and b"two noise levels" in msg
    # valid records, with and without noise, with and without a table: the NULL engine is next
    for e, k, g in ((ok_e, keys, None), (None, None, None), (None, None, np.full((2, 5), 3.0, dtype=np.float32))):
        rc, msg = call(ok_s, e=e, k=k, g=g)
        assert rc == 1 and b"null" in msg, msg
    # the engine-free debug entry
    one = np.array([6.0], dtype=np.float32)
    dbg = lambda cond, g, shape, batch, img: (L.tld_debug_guidance_shape(cond, cond, None, fp(g), fp(shape), batch, img, cond, cond, cond, None), L.tld_last_error())
    here = C.c_void_p(16)                                                      # (never dereferenced: every call below is refused first)
    assert dbg(None, one, ok_s[:1], 1, 4)[0] == 1 and b"null" in L.tld_last_error()
    assert dbg(here, None, ok_s[:1], 1, 4)[0] == 1 and b"null" in L.tld_last_error()
    assert dbg(here, one, None, 1, 4)[0] == 1 and b"null" in L.tld_last_error()
    assert dbg(here, one, ok_s[:1], 0, 4)[0] == 1 and b"positive" in L.tld_last_error()
    assert dbg(here, one, ok_s[:1], 1, 0)[0] == 1 and b"positive" in L.tld_last_error()
    assert dbg(here, one, ok_s[:1], 1, -4)[0] == 1 and b"positive" in L.tld_last_error()
    assert dbg(here, np.array([np.nan], np.float32), ok_s[:1], 1, 4)[0] == 1 and b"guidance" in L.tld_last_error()
    assert dbg(here, one, np.array([[1, 0, 0, 2.0]], np.float32), 1, 4)[0] == 1 and b"phi" in L.tld_last_error()
    assert dbg(here, one, ok_s[1:], 1, 4)[0] == 1 and b"momentum buffer" in L.tld_last_error()       # beta != 0 without the buffer


# ---- 6. the reference loop ------------------------------------------------------------------------------------------------------------------------------
def test_reference_loop_with_neutral_rows_is_the_stochastic_reference_and_a_shape_moves_only_its_request():
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import schedule
    g = load_golden("g1_tiny32_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    ref = TorchRefDenoiser(asdict(cfg), synth_weights(cfg, g["weight_seed"], g["weight_checksum"]))
    gen = torch.Generator().manual_seed(92)
    B = 3
    eps, z0 = torch.randn(B, 4, 32, 32, generator=gen), torch.randn(B, 4, 32, 32, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    neg = [None, torch.randn(768, generator=gen) * 0.5, None]
    mask = torch.ones(B, 1, 32, 32)
    mask[2, :, 4:20, 8:30] = 0
    levels = [schedule.noise_schedule(n, 1) for n in (4, 3, 4)]
    mix, plus, eta = [1.0] * B, [True, False, True], [0.0, 1.0, 0.0]
    gd = [[3.0] * 4, [4.5, 1.0, 4.5], [1.0, 2.0, 2.0, 2.0]]
    z = [[torch.randn(4, 32, 32, generator=gen) for _ in lv[:-1]] for lv in levels]
    args = (ref, eps, z0, mask, labels, neg, levels, mix, gd, plus, eta, z)
    want = S.sample_requests(*args, 0.1, 0.1, trace=True)
    got = R.sample_requests(*args, [R.NEUTRAL] * B, 0.1, 0.1, trace=True)
    for a, w in zip(got, want):
        assert torch.equal(a, w), "neutral rows differ from stochastic_ref"
    one = R.sample_requests(*args, [R.NEUTRAL, R.NEUTRAL, (0.0, 2.5, -0.5, 0.7)], 0.1, 0.1, trace=True)
    assert torch.equal(one[0][:2], want[0][:2]) and not torch.equal(one[0][2], want[0][2])
    # request 2 is unguided at forward 0: x0 = cond there whatever the row says, and the momentum starts at forward 1
    assert torch.equal(one[1][0, 2], want[1][0, 2]) and not torch.equal(one[1][1, 2], want[1][1, 2])
    # the float64 mode follows the float32 one closely and is float64
    dbl = R.sample_requests(*args, [R.NEUTRAL, (1.0, 0.0, 0.0, 1.0), (0.0, 2.5, -0.5, 0.7)], 0.1, 0.1, trace=True, dtype=torch.float64)
    sgl = R.sample_requests(*args, [R.NEUTRAL, (1.0, 0.0, 0.0, 1.0), (0.0, 2.5, -0.5, 0.7)], 0.1, 0.1, trace=True)
    assert dbl[0].dtype == torch.float64 and sgl[0].dtype == torch.float32
    rel = float((dbl[0] - sgl[0].double()).pow(2).mean().sqrt() / dbl[0].pow(2).mean().sqrt())
    print(f"reference loop: float32 against float64 mode, end latent rel-rms {rel:.2e}")
    assert rel < 1e-3
    # the first shaped prediction of the loop is the direct statement on that forward's (c, u)
    lat1 = R.sample_requests(ref, eps[:1], None, None, labels[:1], None, levels[:1], [1.0], [[6.0] * 4], [True], [0.0], None, [(1.0, 0.0, 0.0, 0.0)], trace=True)
    x = eps[:1]
    pair = ref.forward(torch.cat([x, x]), torch.full((2, 1), float(levels[0][0])), torch.stack([labels[0], torch.zeros(768)]))
    c, u = pair[0].numpy(), pair[1].numpy()
    assert torch.equal(lat1[1][0, 0], 6.0 * pair[0] + (1 - 6.0) * pair[1])
    row = (0.0, 2.5, 0.0, 0.7)
    shaped1 = R.sample_requests(ref, eps[:1], None, None, labels[:1], None, levels[:1], [1.0], [[6.0] * 4], [True], [0.0], None, [row], trace=True,
                                dtype=torch.float64)
    want0 = R.direct_f64(c, c.astype(np.float64) - u.astype(np.float64), 6.0, row).reshape(c.shape)      # (the float64 mode does not round d)
    err = float(np.abs(shaped1[1][0, 0].numpy() - want0).max() / np.abs(want0).max())
    print(f"reference loop: first shaped prediction against the direct statement {err:.2e}")
    assert err < 1e-12

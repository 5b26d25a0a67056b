"""CPU: the host side of per-step guidance (tld_sample_requests_guided) -- the guidance table of an interval, the
planning of the unconditional subset the engine repeats in C, the CPU reference loop against tests/requests_ref.py, the refusals (the C ABI's
own before any HIP call, and Python's), the two ABI symbols, and the sort and un-sort of the tables around a stand-in library."""
import ctypes as C
import os
import re
from dataclasses import asdict

import numpy as np
import pytest
import torch

import guided_ref as G
import requests_ref as R
from conftest import cfg_from_arr, load_golden, synth_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- guidance_table ------------------------------------------------------------------------------------------------------------------
def test_guidance_table_interval_edges_and_schedules():
    from transformer_latent_diffusion_amd import schedule
    co = schedule.step_coefficients(schedule.noise_schedule(8, 1))
    sig = co[:, 0]
    assert sig.dtype == np.float32 and len(sig) == 8
    # the edges are inclusive, compared in float32 with the sigma the model is conditioned on
    t = schedule.guidance_table(co, 4.5, (float(sig[5]), float(sig[2])))
    assert t.dtype == np.float32 and t.tolist() == [1.0, 1.0, 4.5, 4.5, 4.5, 4.5, 1.0, 1.0]
    # just inside the edges: the edge levels drop out
    t = schedule.guidance_table(co, 4.5, (float(np.nextafter(sig[5], np.float32(1))), float(np.nextafter(sig[2], np.float32(0)))))
    assert t.tolist() == [1.0, 1.0, 1.0, 4.5, 4.5, 1.0, 1.0, 1.0]
    # an interval outside every level: all ones; None and the whole range: guided throughout; the final prediction's entry is covered
    assert schedule.guidance_table(co, 4.5, (2.0, 3.0)).tolist() == [1.0] * 8
    assert schedule.guidance_table(co, 4.5, None).tolist() == [4.5] * 8 == schedule.guidance_table(co, 4.5, (0.0, 1.0)).tolist()
    assert schedule.guidance_table(co, 4.5, (0.0, float(sig[-1]))).tolist() == [1.0] * 7 + [4.5]
    assert schedule.guidance_table(co, 4.5, (float(sig[0]), 1.0)).tolist() == [4.5] + [1.0] * 7
    # a DDIM schedule has the same levels; an exponent-2 schedule has its own
    ddim = schedule.step_coefficients(schedule.noise_schedule(8, 1), use_ddpm_plus=False)
    assert schedule.guidance_table(ddim, 3.0, (0.3, 0.8)).tolist() == schedule.guidance_table(co, 3.0, (0.3, 0.8)).tolist()
    e2 = schedule.step_coefficients(schedule.noise_schedule(8, 2))
    want = [3.0 if np.float32(0.3) <= s <= np.float32(0.8) else 1.0 for s in e2[:, 0]]
    assert schedule.guidance_table(e2, 3.0, (0.3, 0.8)).tolist() == want and 1.0 in want and 3.0 in want
    assert want != schedule.guidance_table(co, 3.0, (0.3, 0.8)).tolist()
    # a truncated (strength) schedule: the table has the remaining levels only, and entry 0 belongs to the entry level
    k, lv = schedule.truncate_levels(schedule.noise_schedule(8, 1), 0.65)
    tr = schedule.step_coefficients(lv)
    t = schedule.guidance_table(tr, 6.0, (0.3, 0.8))
    assert k == 3 and len(t) == 8 - k and t.tolist() == [6.0 if np.float32(0.3) <= s <= np.float32(0.8) else 1.0 for s in tr[:, 0]]
    assert t[0] == 6.0 and t[-1] == 1.0
    for bad in ((0.8, 0.3), (float("nan"), 0.5)):
        with pytest.raises(ValueError):
            schedule.guidance_table(co, 3.0, bad)
    with pytest.raises(ValueError):
        schedule.guidance_table(co, float("inf"), (0.1, 0.5))
    with pytest.raises(ValueError):
        schedule.guidance_table(co[:, :5], 3.0, (0.1, 0.5))


# ---- guided_rows ---------------------------------------------------------------------------------------------------------------------
def test_guided_rows_plans_the_unconditional_subset():
    from transformer_latent_diffusion_amd import schedule
    counts = [5, 9, 5, 3]
    order = schedule.request_order(counts)
    sc = [counts[b] for b in order]                               # [9, 5, 5, 3]: caller's requests 1, 0, 2, 3
    assert order == [1, 0, 2, 3] and schedule.active_prefix(sc) == [4, 4, 4, 3, 3, 1, 1, 1, 1]
    g = np.float32(3.0)
    tabs = [np.full(9, 1.0, np.float32), np.full(5, 1.0, np.float32), np.full(5, 1.0, np.float32), np.full(3, 1.0, np.float32)]
    tabs[0][[0, 1, 3, 8]] = g          # sorted request 0: guided at steps 0, 1, 3 and on its final prediction
    tabs[1][[0]] = g                   # sorted request 1: step 0 only
    tabs[2][[0, 1, 3, 4]] = g          # sorted request 2: steps 0, 1, 3 and its final prediction (step 4)
    tabs[3][[0]] = g                   # sorted request 3: step 0 only; its final step (2) is unguided
    U, slots, src = schedule.guided_rows(sc, tabs)
    assert U == [4, 2, 0, 2, 1, 0, 0, 0, 1]
    assert slots[0] == [0, 1, 2, 3] and src[0] == [0, 1, 2, 3, 0, 1, 2, 3]                  # U_i = B_i: the mirror
    assert slots[1] == [0, -1, 1, -1] and src[1] == [0, 1, 2, 3, 0, 2]                      # requests 0 and 2 only: a non-prefix subset
    assert slots[2] == [-1, -1, -1, -1] and src[2] == [0, 1, 2, 3]                          # U_i = 0
    assert slots[3] == [0, -1, 1] and src[3] == [0, 1, 2, 0, 2]                             # an odd B_i + U_i
    assert slots[4] == [-1, -1, 0] and src[4] == [0, 1, 2, 2]
    assert slots[8] == [0] and src[8] == [0, 0]
    assert sum(U) == 10 and sum(sc) + sum(U) == 32                                          # model-sample forwards, against 2 x 22 = 44
    assert max(b + u for b, u in zip(schedule.active_prefix(sc), U)) == 8
    # skip off: every request keeps its unconditional sample
    U0, slots0, src0 = schedule.guided_rows(sc, tabs, skip=False)
    assert U0 == schedule.active_prefix(sc) and slots0[1] == [0, 1, 2, 3] and src0[4] == [0, 1, 2, 0, 1, 2]
    # all ones: no unconditional sample anywhere, the engine is B wide
    U1, _, src1 = schedule.guided_rows(sc, [np.ones(c, np.float32) for c in sc])
    assert U1 == [0] * 9 and src1[0] == [0, 1, 2, 3]
    for bad in (tabs[:3], [tabs[0][:8]] + tabs[1:]):
        with pytest.raises(ValueError):
            schedule.guided_rows(sc, bad)
    with pytest.raises(ValueError):
        schedule.guided_rows(counts, [np.ones(c, np.float32) for c in counts])              # not in the engine's order


# ---- the CPU reference ---------------------------------------------------------------------------------------------------------------
def _tiny_ref():
    from oracle.torch_ref import TorchRefDenoiser
    g = load_golden("g1_tiny32_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    return cfg, TorchRefDenoiser(asdict(cfg), synth_weights(cfg, g["weight_seed"], g["weight_checksum"]))


def test_guided_reference_equals_the_requests_reference():
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    gen = torch.Generator().manual_seed(71)
    B = 3
    eps, z0 = torch.randn(B, 4, 32, 32, generator=gen), torch.randn(B, 4, 32, 32, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    neg = [None, torch.randn(768, generator=gen) * 0.5, None]
    mask = torch.ones(B, 1, 32, 32)
    mask[2, :, 4:20, 8:30] = 0
    n_iter, strength, g, plus = [4, 3, 6], [None, None, 0.65], [3.0, 4.5, 2.0], [True, False, True]
    levels, mix = [], []
    for b in range(B):
        lv = schedule.noise_schedule(n_iter[b], 1)
        k = 0
        if strength[b] is not None:
            k, lv = schedule.truncate_levels(lv, strength[b])
        levels.append(lv)
        mix.append(float(np.float32(lv[0])) if k > 0 else 1.0)
    args = (ref, eps, z0, mask, labels, neg, levels, mix)
    want = R.sample_requests(*args, g, plus, 0.1, 0.1, trace=True)
    got = G.sample_requests(*args, [[g[b]] * len(levels[b]) for b in range(B)], plus, 0.1, 0.1, trace=True)
    for a, w in zip(got, want):
        assert torch.equal(a, w), "constant tables differ from requests_ref"
    # all ones against guidance 1 of requests_ref: the formula at g = 1 is the value up to the sign of a zero, hence ==
    want1 = R.sample_requests(*args, [1.0] * B, plus, 0.1, 0.1, trace=True)
    got1 = G.sample_requests(*args, [[1.0] * len(levels[b]) for b in range(B)], plus, 0.1, 0.1, trace=True)
    for a, w in zip(got1, want1):
        assert bool((a == w).all()), "all-ones tables differ from requests_ref at guidance 1"
    # an interval moves the result, and only from the first forward it changes on
    tabs = [[g[b]] * len(levels[b]) for b in range(B)]
    tabs[0][2] = 1.0
    mixed = G.sample_requests(*args, tabs, plus, 0.1, 0.1, trace=True)
    assert torch.equal(mixed[1][:2, 0], want[1][:2, 0]) and not torch.equal(mixed[1][2, 0], want[1][2, 0])
    assert torch.equal(mixed[0][1:], want[0][1:]) and not torch.equal(mixed[0][0], want[0][0])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_guided_calls_before_any_hip_call():
    """The record checks of tld_sample_requests_guided need neither an engine nor a device, so they come first: a NULL table, an entry that
    is not finite, an order violation and a level count below 2 are refused with TLD_ERR_INVALID; a record's class_guidance is ignored."""
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    Rq = _lib.TldSampleRequest
    tab = np.zeros((2, 5, 6), dtype=np.float32)
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))

    def call(r0, r1, g, n_max=5):
        recs = (Rq * 2)(r0, r1)
        return L.tld_sample_requests_guided(None, None, None, None, None, None, recs, fp(tab), fp(g), n_max, 0.0, 0.0, None, 2, None, None, None)

    ok = np.full((2, 5), 3.0, dtype=np.float32)
    assert call(Rq(5, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 0), None) == 1 and b"null" in L.tld_last_error()
    bad = ok.copy(); bad[1, 2] = np.inf
    assert call(Rq(5, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 0), bad) == 1 and b"request 1" in L.tld_last_error() and b"forward 2" in L.tld_last_error()
    bad = ok.copy(); bad[0, 4] = np.nan
    assert call(Rq(5, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 0), bad) == 1 and b"not finite" in L.tld_last_error()
    assert call(Rq(3, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 0), ok) == 1 and b"non-increasing" in L.tld_last_error()
    assert call(Rq(5, 1.0, 1.0, 0), Rq(1, 1.0, 1.0, 0), ok) == 1 and b"two noise levels" in L.tld_last_error()
    assert call(Rq(5, 1.0, 0.0, 0), Rq(5, 1.0, 1.0, 0), ok) == 1 and b"start_mix" in L.tld_last_error()
    past = ok.copy(); past[1, 3:] = np.nan                        # entries past n_levels are ignored, and so is class_guidance
    assert call(Rq(5, float("nan"), 1.0, 0), Rq(3, 1.0, 1.0, 0), past) == 1 and b"null" in L.tld_last_error()    # valid: the NULL engine is next
    c, u = C.c_int64(), C.c_int64()
    assert L.tld_engine_sample_rows(None, C.byref(c), C.byref(u)) == 1 and b"null" in L.tld_last_error()


class _FakeLib:
    """Stands in for libtld_hip.so: records what tld_sample_requests_guided receives and writes into out_latent[k] a value that names the
    record's table -- through host pointers (the tensors are CPU ones)."""

    def __init__(self, img):
        self.img, self.calls = img, []

    def tld_sample_requests_guided(self, h, eps, z0, m, lab, neg, recs, table, guid, n_max, sharp, bright, out, B, tx0, txt, stream):
        recs = [(r.n_levels, r.class_guidance, r.start_mix, r.has_negative) for r in recs]
        assert all(recs[k][0] >= recs[k + 1][0] for k in range(B - 1)), "records not ordered by non-increasing n_levels"
        g = np.ctypeslib.as_array(guid, shape=(B, n_max)).copy()
        self.calls.append(dict(recs=recs, g=g, n_max=n_max, B=B, entry="guided"))
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(B, self.img))
        for k in range(B):
            o[k] = g[k, 0] * 100 + recs[k][0]
        return 0

    def tld_sample_requests(self, *a):
        self.calls.append(dict(entry="plain"))
        return 0


def _fake_denoiser(monkeypatch, engine=None):
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, _lib
    m = Denoiser(**asdict(DenoiserConfig(n_channels=4)))
    fake = _FakeLib(4 * 16 * 16)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(_lib, "check", lambda rc, what: None)
    monkeypatch.setattr(m, "_resolve_device", lambda t=None: torch.device("cpu"))
    monkeypatch.setattr(m, "_ensure_engine", lambda n, dev: None if engine is None else engine.append(n))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 0})())
    monkeypatch.setattr(torch.cuda, "device", lambda dev: __import__("contextlib").nullcontext())
    return m, fake


def test_guidance_steps_are_sorted_and_unsorted_with_the_requests(monkeypatch):
    from transformer_latent_diffusion_amd import schedule
    engine = []
    m, fake = _fake_denoiser(monkeypatch, engine)
    monkeypatch.delenv("TLD_GUIDANCE_SKIP", raising=False)
    counts = [5, 9, 5, 3]
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1)) for n in counts]
    steps = [np.full(n, float(b + 2), np.float32) for b, n in enumerate(counts)]
    steps[0][1:] = 1.0
    steps[3][:] = 1.0
    out = m.sample_latents_requests(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), coeffs, None, guidance_steps=steps)
    call = fake.calls[0]
    assert call["entry"] == "guided" and [r[0] for r in call["recs"]] == [9, 5, 5, 3] and call["g"].shape == (4, 9)
    for k, b in enumerate([1, 0, 2, 3]):
        assert call["g"][k, :counts[b]].tolist() == steps[b].tolist() and not call["g"][k, counts[b]:].any()      # padded with zeros past n_levels
        assert float(out[b, 0, 0, 0]) == float(steps[b][0]) * 100 + counts[b]                                     # back in the caller's order
    # the engine is ensured for the largest step: step 0 runs 4 requests and the 3 guided ones
    assert engine == [7]
    monkeypatch.setenv("TLD_GUIDANCE_SKIP", "0")
    m.sample_latents_requests(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), coeffs, None, guidance_steps=steps)
    assert engine == [7, 8]
    monkeypatch.delenv("TLD_GUIDANCE_SKIP")
    m.sample_latents_requests(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), coeffs, None, guidance_steps=[np.ones(n, np.float32) for n in counts])
    assert engine == [7, 8, 4]
    # without tables the entry is the old one, CFG-doubled
    m.sample_latents_requests(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), coeffs, [3.0] * 4)
    assert fake.calls[-1]["entry"] == "plain" and engine[-1] == 8


def test_python_refusals(monkeypatch):
    from transformer_latent_diffusion_amd import DiffusionGenerator, RequestBatcher, schedule
    m, fake = _fake_denoiser(monkeypatch)
    gen = DiffusionGenerator(m, None, torch.device("cpu"), torch.float32)
    lab = torch.zeros(3, 768)
    ok = dict(n_iter=[4, 5, 6], class_guidance=3.0, seed=1, img_size=16)
    gen.generate_latents_requests(lab, guidance_interval=(0.2, 0.8), **ok)
    gen.generate_latents_requests(lab, guidance_interval=[(0.2, 0.8), None, (0.0, 1.0)], **ok)
    gen.generate_latents_requests(lab, guidance_schedule=[np.ones(4), None, np.full(6, 2.0)], **ok)
    assert [c["entry"] for c in fake.calls] == ["guided"] * 3
    # the schedule wins over the interval and the scalar; a request without either keeps the scalar throughout
    g = fake.calls[2]["g"]                                          # engine order: 6, 5, 4 levels
    assert g[0, :6].tolist() == [2.0] * 6 and g[1, :5].tolist() == [3.0] * 5 and g[2, :4].tolist() == [1.0] * 4
    co5 = schedule.step_coefficients(schedule.noise_schedule(5, 1))
    assert fake.calls[1]["g"][1, :5].tolist() == [3.0] * 5 and fake.calls[0]["g"][1, :5].tolist() == schedule.guidance_table(co5, 3.0, (0.2, 0.8)).tolist()
    bad = [dict(guidance_interval=(0.8, 0.2)), dict(guidance_interval=[(0.2, 0.8), (0.9, 0.1), None]), dict(guidance_interval=[(0.2, 0.8)] * 2),
           dict(guidance_interval=(0.1, 0.2, 0.3)), dict(guidance_schedule=[np.ones(4), np.ones(4), np.ones(6)]), dict(guidance_schedule=[np.ones(4)] * 2),
           dict(guidance_schedule=[np.ones(4), np.full(5, np.nan), None])]
    for kw in bad:
        with pytest.raises(ValueError):
            gen.generate_latents_requests(lab, **dict(ok, **kw))
    co = [schedule.step_coefficients(schedule.noise_schedule(4, 1))] * 3
    for steps in ([np.ones(4)] * 2, [np.ones(4), np.ones(3), np.ones(4)], [np.ones(4), np.full(4, np.inf), np.ones(4)], [np.ones((4, 1))] * 3):
        with pytest.raises(ValueError):
            m.sample_latents_requests(torch.zeros(3, 4, 16, 16), lab, co, None, guidance_steps=steps)
    assert len(fake.calls) == 3, "a refused call reached the engine"
    # the uniform entries route an interval to the requests path; None keeps them where they are
    gen.generate_latents(lab, n_iter=4, num_imgs=3, class_guidance=3.0, img_size=16, guidance_interval=(0.2, 0.8))
    assert fake.calls[-1]["entry"] == "guided" and fake.calls[-1]["B"] == 3
    with pytest.raises(ValueError):
        gen.generate_latents(lab, n_iter=4, num_imgs=3, class_guidance=3.0, img_size=16, guidance_interval=(0.8, 0.2))

    class Pipe:
        def __init__(self):
            self.calls = []

        def generate_images_from_texts(self, prompts, **kw):
            self.calls.append(kw)
            return list(prompts)

    with pytest.raises(ValueError, match="mixed=True"):
        RequestBatcher(Pipe(), mixed=False).submit("a", guidance_interval=(0.2, 0.8))
    with pytest.raises(ValueError):
        RequestBatcher(Pipe(), mixed=True).submit("a", guidance_interval=(0.8, 0.2))
    pipe = Pipe()
    rb = RequestBatcher(pipe, max_batch=4, mixed=True)
    t = [rb.submit("a", 6, 1, 15, guidance_interval=(0.2, 0.8)), rb.submit("b", 3, 2, 15)]
    assert rb.flush() == {t[0]: "a", t[1]: "b"} and pipe.calls[0]["guidance_interval"] == [(0.2, 0.8), None]
    rb.submit("c", 3, 2, 15)
    rb.flush()
    assert "guidance_interval" not in pipe.calls[1]                 # no interval in the call: the keyword is not passed


def test_abi_symbols_in_header_exports_and_list():
    from transformer_latent_diffusion_amd import Denoiser, _lib
    hdr = open(os.path.join(REPO, "include", "tld_hip.h")).read()
    for sym in ("tld_sample_requests_guided", "tld_engine_sample_rows"):
        assert re.search(r"TLD_API\s+int\s+" + sym + r"\s*\(", hdr) and sym in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), sym)
    bits = int(re.search(r"#define TLD_ENGINE_PATH_BITS (\d+)", hdr).group(1))
    assert bits == 61 and sorted(Denoiser.SAMPLER_PATH_NAMES) == [58, 59, 60]            # no new path bits
    assert C.sizeof(_lib.TldSampleRequest) == 16

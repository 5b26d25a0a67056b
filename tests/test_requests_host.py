"""CPU: the host side of the per-request sampler call (tld_sample_requests) -- the sort and un-sort around the
engine's record order, the active prefixes, the deduplicated noise rows, the row cap of the mixed request planner, the argument refusals
(Python's, and the C ABI's own before any HIP call), the ABI symbol, and the CPU reference the GPU tests compare with
(tests/requests_ref.py), pinned per request to tests/img2img_ref.py."""
import ctypes as C
import os
import re
from dataclasses import asdict

import numpy as np
import pytest
import torch

import img2img_ref as R1
import requests_ref as R
from conftest import cfg_from_arr, load_golden, synth_weights

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- sorting, prefixes, rows ---------------------------------------------------------------------------------------------------------
def test_request_order_and_active_prefix():
    from transformer_latent_diffusion_amd import schedule
    counts = [5, 9, 5, 3]
    order = schedule.request_order(counts)
    assert order == [1, 0, 2, 3]                                  # descending, equal counts keep the caller's order
    sorted_counts = [counts[b] for b in order]
    assert sorted_counts == [9, 5, 5, 3]
    assert schedule.active_prefix(sorted_counts) == [4, 4, 4, 3, 3, 1, 1, 1, 1]
    assert sum(schedule.active_prefix(sorted_counts)) == sum(counts)          # model-sample forwards / 2: a finished request is not computed again
    with pytest.raises(ValueError):
        schedule.active_prefix(counts)
    assert schedule.request_order([]) == [] and schedule.active_prefix([]) == []


class _FakeLib:
    """Stands in for libtld_hip.so: records what tld_sample_requests receives, checks the record order as the engine does, and writes
    into out_latent[k] / the trace slots a value that names the record's guidance -- through host pointers (the tensors are CPU ones)."""

    def __init__(self, img):
        self.img, self.calls = img, []

    def tld_sample_requests(self, h, eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream):
        recs = [(r.n_levels, r.class_guidance, r.start_mix, r.has_negative) for r in recs]
        assert all(recs[k][0] >= recs[k + 1][0] for k in range(B - 1)), "records not ordered by non-increasing n_levels"
        tab = np.ctypeslib.as_array(table, shape=(B, n_max, 6)).copy()
        self.calls.append(dict(recs=recs, table=tab, n_max=n_max, B=B, has_z0=z0.value is not None, has_mask=m.value is not None,
                               has_neg=neg.value is not None))
        o = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_float)), shape=(B, self.img))
        for k in range(B):
            o[k] = recs[k][1] * 100 + recs[k][0]
        if tx0.value is not None:
            t = np.ctypeslib.as_array(C.cast(tx0, C.POINTER(C.c_float)), shape=(n_max - 1, B, self.img))
            for k in range(B):
                t[: recs[k][0] - 1, k] = recs[k][1]
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


def test_sample_latents_requests_sorts_and_unsorts(monkeypatch):
    from transformer_latent_diffusion_amd import schedule
    m, fake = _fake_denoiser(monkeypatch)
    counts, guid = [5, 9, 5, 3], [1.0, 2.0, 3.0, 4.0]
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1)) for n in counts]
    out, tx0, txt = m.sample_latents_requests(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), coeffs, guid, trace=True)
    call = fake.calls[0]
    assert [r[0] for r in call["recs"]] == [9, 5, 5, 3] and [r[1] for r in call["recs"]] == [2.0, 1.0, 3.0, 4.0]
    assert call["n_max"] == 9 and call["table"].shape == (4, 9, 6)
    assert np.array_equal(call["table"][0], coeffs[1]) and np.array_equal(call["table"][1, :5], coeffs[0])
    assert not call["table"][1, 5:].any() and np.array_equal(call["table"][3, :3], coeffs[3])          # padded with zeros past n_levels
    assert not (call["has_z0"] or call["has_mask"] or call["has_neg"])
    # results come back in the caller's order
    for b in range(4):
        assert float(out[b, 0, 0, 0]) == guid[b] * 100 + counts[b]
        assert tx0.shape == (8, 4, 4, 16, 16)
        assert bool((tx0[: counts[b] - 1, b] == guid[b]).all()) and not tx0[counts[b] - 1:, b].any()   # a finished request's slots stay zero


def test_sigma_rows_are_deduplicated_by_value():
    from transformer_latent_diffusion_amd import schedule
    a = schedule.step_coefficients(schedule.noise_schedule(8, 1))
    c = schedule.step_coefficients(schedule.noise_schedule(5, 1))
    sig, rows = schedule.distinct_sigma_rows([a, a.copy(), c])
    # 8 levels + 5 levels share only 0.99: 8 + 4 rows; an identical schedule adds none
    shared = len(set(a[:, 0].tolist()) & set(c[:, 0].tolist()))
    assert shared == 1 and len(sig) == 8 + 5 - shared
    assert rows[0] == rows[1] and len(rows[2]) == 5 and rows[2][0] == rows[0][0]
    for b, t in enumerate((a, a, c)):
        assert [float(sig[r]) for r in rows[b]] == t[:, 0].tolist()          # the tables index the right sigma
    assert len(set(sig.tolist())) == len(sig)
    assert schedule.request_cond_rows([a, a, c], n_negative=2) == len(sig) + 3 + 1 + 2
    # two unrelated schedules: n + n' rows
    d = schedule.step_coefficients(schedule.noise_schedule(7, 2))
    assert len(schedule.distinct_sigma_rows([a, a, d])[0]) == 8 + 7 - len(set(a[:, 0].tolist()) & set(d[:, 0].tolist()))


# ---- the mixed planner ---------------------------------------------------------------------------------------------------------------
class FakePipe:
    def __init__(self):
        self.calls = []

    def generate_images_from_texts(self, prompts, class_guidance, seeds, n_iter, negative_prompts=None):
        self.calls.append((list(prompts), class_guidance, list(seeds), n_iter, negative_prompts))
        return [f"img:{p}:{s}" for p, s in zip(prompts, seeds)]


def test_mixed_request_batcher_fills_calls_in_submission_order():
    from transformer_latent_diffusion_amd import RequestBatcher
    pipe = FakePipe()
    rb = RequestBatcher(pipe, max_batch=2, mixed=True)
    t = [rb.submit("a", 6, 1, 15), rb.submit("b", 3, 2, 15), rb.submit("c", 6, 3, 15), rb.submit("d", 6, 4, 15),
         rb.submit("e", 6, 5, 30, negative_prompt="blurry")]
    assert rb.pending() == 5
    plan = rb.plan()
    assert [[r[1] for r in call] for call in plan] == [["a", "b"], ["c", "d"], ["e"]]
    out = rb.flush()
    assert out == {t[0]: "img:a:1", t[1]: "img:b:2", t[2]: "img:c:3", t[3]: "img:d:4", t[4]: "img:e:5"}
    assert rb.pending() == 0 and rb.flush() == {}
    assert pipe.calls == [(["a", "b"], [6.0, 3.0], [1, 2], [15, 15], None), (["c", "d"], [6.0, 6.0], [3, 4], [15, 15], None),
                          (["e"], [6.0], [5], [30], ["blurry"])]
    # the default planner is unchanged and refuses what it cannot serve
    rb0 = RequestBatcher(FakePipe(), max_batch=2)
    with pytest.raises(ValueError):
        rb0.submit("a", negative_prompt="x")


def test_mixed_planner_row_cap_arithmetic():
    from transformer_latent_diffusion_amd import RequestBatcher, schedule
    assert schedule.REQUEST_ROW_CAP == 1024
    # 15 and 30 levels: n / 15 = 2 n / 30 share every level but those that round differently in float32; count them by value
    s15 = set(np.asarray(schedule.noise_schedule(15, 1), dtype=np.float32).tolist())
    s30 = set(np.asarray(schedule.noise_schedule(30, 1), dtype=np.float32).tolist())
    assert RequestBatcher.call_rows([(15, False)]) == 15 + 1 + 1
    assert RequestBatcher.call_rows([(15, False), (15, True)]) == 15 + 2 + 1 + 1
    assert RequestBatcher.call_rows([(15, False), (30, False)]) == len(s15 | s30) + 2 + 1
    # requests with pairwise different n_iter: a call is cut where the next request would pass the cap, not at max_batch
    rb = RequestBatcher(FakePipe(), max_batch=64, mixed=True)
    n_its = list(range(40, 80))
    for i, n in enumerate(n_its):
        rb.submit(f"p{i}", 6, i, n)
    plan = rb.plan()
    assert len(plan) > 1 and sum(len(c) for c in plan) == len(n_its)
    for k, call in enumerate(plan):
        rows = RequestBatcher.call_rows([(r[4], r[5] is not None) for r in call])
        assert rows <= schedule.REQUEST_ROW_CAP
        if k + 1 < len(plan):
            nxt = plan[k + 1][0]
            assert RequestBatcher.call_rows([(r[4], r[5] is not None) for r in call + [nxt]]) > schedule.REQUEST_ROW_CAP
    assert [r[0] for call in plan for r in call] == list(range(len(n_its)))         # submission order


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_on_the_host(monkeypatch):
    from transformer_latent_diffusion_amd import DiffusionGenerator, schedule
    m, fake = _fake_denoiser(monkeypatch)
    gen = DiffusionGenerator(m, None, torch.device("cpu"), torch.float32)
    lab = torch.zeros(3, 768)
    ok = dict(n_iter=[4, 5, 6], class_guidance=3.0, seed=1, img_size=16)
    gen.generate_latents_requests(lab, **ok)
    assert len(fake.calls) == 1
    bad = [dict(n_iter=[4, 5]), dict(class_guidance=[1.0, 2.0]), dict(n_iter=[4, 1, 6]), dict(class_guidance=[1.0, float("nan"), 2.0]),
           dict(class_guidance=float("inf")), dict(negative_labels=torch.zeros(3, 767)), dict(negative_labels=torch.zeros(2, 768)),
           dict(negative_labels=[None, torch.zeros(5), None]), dict(strength=[None, 0.5, None]), dict(mask=torch.ones(3, 1, 16, 16)),
           dict(init_latents=torch.zeros(3, 4, 16, 16), strength=[0.5, 1.5, None]), dict(init_latents=torch.zeros(2, 4, 16, 16)),
           dict(init_latents=torch.zeros(3, 4, 16, 16), mask=torch.full((3, 1, 16, 16), 2.0)), dict(seeds=[1, 2]), dict(exponent=[1, 2])]
    for kw in bad:
        with pytest.raises(ValueError):
            gen.generate_latents_requests(lab, **dict(ok, **kw))
    assert len(fake.calls) == 1, "a refused call reached the engine"
    co = [schedule.step_coefficients(schedule.noise_schedule(4, 1))] * 3
    for kw in (dict(guidance=[1.0, 2.0]), dict(guidance=[1.0, 2.0, float("nan")]), dict(start_mix=[1.0, 0.0, 1.0]), dict(start_mix=[1.0, 0.5, 1.0]),
               dict(coeffs=co[:2]), dict(coeffs=[co[0], co[0][:1], co[0]]), dict(neg_labels=torch.zeros(3, 5))):
        with pytest.raises(ValueError):
            m.sample_latents_requests(torch.zeros(3, 4, 16, 16), lab, kw.get("coeffs", co), kw.get("guidance", [1.0] * 3),
                                      start_mix=kw.get("start_mix"), neg_labels=kw.get("neg_labels"))
    assert len(fake.calls) == 1


def test_c_abi_refuses_bad_records_before_any_hip_call():
    """The record checks of tld_sample_requests need neither an engine nor a device, so they come first: an order violation, a level
    count below 2, a start_mix outside (0, 1], a guidance that is not finite and a negative flag without neg_labels handed straight to the
    C ABI are refused with TLD_ERR_INVALID and a message that names the request."""
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    Rq = _lib.TldSampleRequest
    tab = np.zeros((2, 5, 6), dtype=np.float32)

    def call(r0, r1, n_max=5):
        recs = (Rq * 2)(r0, r1)
        return L.tld_sample_requests(None, None, None, None, None, None, recs, tab.ctypes.data_as(C.POINTER(C.c_float)), n_max, 0.0, 0.0, None, 2,
                                     None, None, None)

    assert call(Rq(3, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 0)) == 1 and b"non-increasing" in L.tld_last_error()
    assert call(Rq(5, 1.0, 1.0, 0), Rq(1, 1.0, 1.0, 0)) == 1 and b"request 1" in L.tld_last_error() and b"two noise levels" in L.tld_last_error()
    assert call(Rq(5, 1.0, 0.0, 0), Rq(5, 1.0, 1.0, 0)) == 1 and b"start_mix" in L.tld_last_error()
    assert call(Rq(5, 1.0, 1.5, 0), Rq(5, 1.0, 1.0, 0)) == 1 and b"start_mix" in L.tld_last_error()
    assert call(Rq(5, float("nan"), 1.0, 0), Rq(5, 1.0, 1.0, 0)) == 1 and b"class_guidance" in L.tld_last_error()
    assert call(Rq(5, 1.0, 1.0, 0), Rq(5, 1.0, 1.0, 1)) == 1 and b"neg_labels" in L.tld_last_error()
    assert call(Rq(5, 1.0, 0.5, 0), Rq(5, 1.0, 1.0, 0)) == 1 and b"init_latent" in L.tld_last_error()
    assert call(Rq(4, 1.0, 1.0, 0), Rq(4, 1.0, 1.0, 0)) == 1 and b"n_max" in L.tld_last_error()
    assert call(Rq(5, 1.0, 1.0, 0), Rq(3, 1.0, 1.0, 0)) == 1 and b"null" in L.tld_last_error()       # valid records: the NULL engine is next
    assert C.sizeof(Rq) == 16


def test_abi_symbol_in_header_exports_and_list():
    from transformer_latent_diffusion_amd import Denoiser, _lib
    hdr = open(os.path.join(REPO, "include", "tld_hip.h")).read()
    assert re.search(r"TLD_API\s+int\s+tld_sample_requests\s*\(", hdr) and "tld_sample_requests" in _lib.ABI_SYMBOLS
    assert hasattr(_lib.lib(), "tld_sample_requests")
    bits = int(re.search(r"#define TLD_ENGINE_PATH_BITS (\d+)", hdr).group(1))
    assert sorted(Denoiser.SAMPLER_PATH_NAMES) == [58, 59, 60] and bits == 61 and len(Denoiser.PATH_NAMES) == 54


# ---- the CPU reference -----------------------------------------------------------------------------------------------------------
def _tiny_ref():
    from oracle.torch_ref import TorchRefDenoiser
    g = load_golden("g1_tiny32_forward.npz")
    cfg = cfg_from_arr(g["cfg"])
    return cfg, TorchRefDenoiser(asdict(cfg), synth_weights(cfg, g["weight_seed"], g["weight_checksum"]))


def test_reference_loop_equals_the_solo_reference_per_request():
    from transformer_latent_diffusion_amd import schedule
    cfg, ref = _tiny_ref()
    gen = torch.Generator().manual_seed(51)
    B = 4
    eps, z0 = torch.randn(B, 4, 32, 32, generator=gen), torch.randn(B, 4, 32, 32, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    mask = torch.ones(B, 1, 32, 32)
    mask[2, :, 4:20, 8:30] = 0
    mask[3] = torch.rand(1, 32, 32, generator=gen)
    n_iter, strength, g, plus = [5, 3, 6, 4], [None, None, 0.65, 1.0], [3.0, 1.0, 4.5, 6.0], [True, True, True, False]
    levels, mix = [], []
    for b in range(B):
        lv = schedule.noise_schedule(n_iter[b], 1)
        k = 0
        if strength[b] is not None:
            k, lv = schedule.truncate_levels(lv, strength[b])
        levels.append(lv)
        mix.append(float(np.float32(lv[0])) if k > 0 else 1.0)
    out, tx0, txt = R.sample_requests(ref, eps, z0, mask, labels, [None, torch.zeros(768), None, None], levels, mix, g, plus, 0.1, 0.1, trace=True)
    worst = 0.0
    for b in range(B):
        s = slice(b, b + 1)
        want, wx0, wxt = R1.sample_from(ref, eps[s], z0[s], mask[s], labels[s], levels[b], mix[b], g[b], plus[b], 0.1, 0.1, trace=True)
        n = len(levels[b]) - 1
        for a, w in ((out[b], want[0]), (tx0[:n, b], wx0[:, 0]), (txt[:n, b], wxt[:, 0])):
            worst = max(worst, float(((a - w).abs().max() / w.abs().max())))
        assert not tx0[n:, b].any() and not txt[n:, b].any()
    print(f"requests_ref vs img2img_ref per request: worst relative difference {worst:.3e} "
          f"({'bitwise equal' if worst == 0.0 else 'not bitwise'})")
    assert worst <= 1e-6
    # a real negative label moves the result, and the batched loop agrees with itself run alone
    neg = [None, torch.randn(768, generator=gen) * 0.5, None, None]
    out2 = R.sample_requests(ref, eps, z0, mask, labels, neg, levels, mix, g, plus, 0.1, 0.1)
    solo = R.sample_requests(ref, eps[1:2], z0[1:2], mask[1:2], labels[1:2], neg[1:2], levels[1:2], mix[1:2], g[1:2], plus[1:2], 0.1, 0.1)
    assert torch.equal(out2[1], solo[0])
    assert torch.equal(out2[1], out[1])                 # g = 1: the unconditional half has weight 0 -> (1 - g) * x = 0 exactly
    g2 = list(g); g2[1] = 3.0
    assert not torch.equal(R.sample_requests(ref, eps, z0, mask, labels, neg, levels, mix, g2, plus)[1],
                           R.sample_requests(ref, eps, z0, mask, labels, None, levels, mix, g2, plus)[1])

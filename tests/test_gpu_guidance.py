"""GPU: one guidance value per forward in the on-device sampler (tld_sample_requests_guided).

A forward whose guidance is exactly 1.0 runs no unconditional model sample and takes x0 = cond.  The defining rule is bitwise: an engine that
skips those samples returns, for every request, what an engine created under TLD_GUIDANCE_SKIP=0 returns, which runs the full CFG-doubled
batch and combines with the fma at g = 1 -- and tld_engine_sample_rows shows that the skipping engine did skip.  Constant tables are today's
tld_sample_requests, bit for bit.  Against the CPU reference loop (tests/guided_ref.py) the project's contract tolerances hold (TRAJ_TOL,
FWD_TOL of tests/test_gpu_requests.py).  Every test prints the figures it asserts."""
import ctypes as C
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

import guided_ref as G
from conftest import cfg_from_arr, load_golden, synth_weights

pytestmark = pytest.mark.gpu

TRAJ_TOL = 6e-2          # the contract tolerance of a multi-step CFG trajectory (tests/test_gpu_parity.py)
FWD_TOL = 2e-2           # ... of one forward

TINY, BIG = "g2_tiny32_sampler.npz", "g5_100m.npz"
FIVE = dict(class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], n_iter=[8, 5, 8, 3, 5], use_ddpm_plus=[True, True, False, True, True],
            exponent=[1, 1, 1, 1, 2])
BIG3 = dict(class_guidance=[6.0, 3.0, 4.5], n_iter=[4, 6, 6], use_ddpm_plus=[True, True, False], exponent=[1, 1, 2])

_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(fixture, low_latency=0, skip=True, share=True, fp8=False, reserve=10):
    """(Denoiser, DiffusionGenerator) for a golden fixture's configuration and synthetic weights, its engine built here for ``reserve``
    samples under the environment switches asked for (they are read at tld_engine_create), so that no later call rebuilds it."""
    key = (fixture, low_latency, skip, share, fp8)
    if key not in _CACHE:
        from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
        g = load_golden(fixture)
        cfg = cfg_from_arr(g["cfg"])
        sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
        m = Denoiser(**asdict(cfg)).to(_dev())
        if low_latency:
            m.set_low_latency(low_latency)
        if fp8:
            m.set_gemm_dtype("fp8")
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        env = {"TLD_GUIDANCE_SKIP": None if skip else "0", "TLD_SHARE_L0": None if share else "0"}
        old = {k: os.environ.get(k) for k in env}
        try:
            for k, v in env.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
            m.reserve(reserve)
        finally:
            for k, v in old.items():
                os.environ.pop(k, None)
                if v is not None:
                    os.environ[k] = v
        assert m._engine_skip == skip
        _CACHE[key] = (m, DiffusionGenerator(m, None, _dev(), torch.float32), cfg, sd)
    m, gen = _CACHE[key][:2]
    assert m._engine is not None and m._engine_skip == skip, "the engine was rebuilt"
    return m, gen


def _inputs(B, S=32, seed=81):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S, S, generator=gen)
    z0 = torch.randn(B, 4, S, S, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


def _rect_mask(S=32):
    m = torch.zeros(1, S, S)
    m[:, 5:21, 3:17] = 1
    return m


def _tab(g, pattern):
    """a guidance table: g where the pattern has 1, exactly 1.0 where it has 0"""
    return np.array([g if p else 1.0 for p in pattern], dtype=np.float32)


def _kw(d):
    return {k: v for k, v in d.items() if k != "class_guidance"}


def _plan(n_iter, tables):
    """the planner's figures of a call in the caller's order: (sum n_levels, U per step, slots per step, largest model batch)"""
    from transformer_latent_diffusion_amd import schedule
    order = schedule.request_order(n_iter)
    sc = [n_iter[b] for b in order]
    U, slots, src = schedule.guided_rows(sc, [tables[b] for b in order])
    return sum(sc), U, slots, max(b + u for b, u in zip(schedule.active_prefix(sc), U))


def _equal3(a, b, what):
    for u, v, name in zip(a, b, ("end latent", "trace_x0", "trace_xt")):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {name} differs"


# ---- 1. constant tables are today's entry ---------------------------------------------------------------------------------------------
def test_constant_tables_equal_todays_entry():
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(5)
    want = gen.generate_latents_requests(labels, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, **FIVE)
    n = sum(FIVE["n_iter"])
    assert m.sample_rows() == (n, n)
    tables = [np.full(k, g, np.float32) for k, g in zip(FIVE["n_iter"], FIVE["class_guidance"])]
    got = gen.generate_latents_requests(labels, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, guidance_schedule=tables, **FIVE)
    _equal3(got, want, "constant tables")
    rows = m.sample_rows()
    print(f"constant tables: sample rows {rows}; today's entry ({n}, {n})")
    assert rows == (n, n - FIVE["n_iter"][0])                       # request 0 is guided at 1.0: its unconditional samples are not run


# ---- 2. all-ones tables are class_guidance = 1 through today's entry, on an engine of B samples -----------------------------------------
@pytest.mark.parametrize("fixture", [TINY, BIG], ids=["tiny", "100m"])
def test_all_ones_tables_equal_guidance_one_and_need_b_samples(fixture):
    from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
    m, gen = _model(fixture)
    B = 5
    eps, z0, labels = _inputs(B, seed=82)
    kw = dict(n_iter=[4, 3, 4, 2, 3], use_ddpm_plus=[True, True, False, True, True], seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True)
    want = gen.generate_latents_requests(labels, class_guidance=1.0, **kw)
    small = Denoiser(**asdict(_CACHE[(fixture, 0, True, True, False)][2])).to(_dev())
    small.load_state_dict(m.state_dict())
    small.reserve(B)
    cap = small._engine_batch
    assert cap < 2 * B
    gen1 = DiffusionGenerator(small, None, _dev(), torch.float32)
    got = gen1.generate_latents_requests(labels, guidance_schedule=[np.ones(n, np.float32) for n in kw["n_iter"]], **kw)
    assert small._engine_batch == cap, "the engine was rebuilt for more samples"
    for u, v, name in zip(got, want, ("end latent", "trace_x0", "trace_xt")):
        assert bool((u == v).all()), f"all-ones tables, {fixture}: {name} differs from class_guidance = 1"
    rows = small.sample_rows()
    print(f"all ones, {fixture}: engine of {cap} samples served {B} requests (2 B = {2 * B}); sample rows {rows}")
    assert rows == (sum(kw["n_iter"]), 0)
    # the same call CFG-doubled does not fit that engine
    with pytest.raises(RuntimeError, match="max_batch"):
        from transformer_latent_diffusion_amd import _lib, schedule
        co = [schedule.step_coefficients(schedule.noise_schedule(2, 1))] * B
        tab = np.stack(co)
        recs = (_lib.TldSampleRequest * B)(*[_lib.TldSampleRequest(2, 1.0, 1.0, 0)] * B)
        x = eps.to(_dev()).contiguous()
        _lib.check(_lib.lib().tld_sample_requests(small._engine, C.c_void_p(x.data_ptr()), None, None, C.c_void_p(labels.to(_dev()).contiguous().data_ptr()),
                                                  None, recs, tab.ctypes.data_as(C.POINTER(C.c_float)), 2, 0.0, 0.0,
                                                  C.c_void_p(torch.empty_like(x).data_ptr()), B, None, None, None), "tld_sample_requests")


# ---- 3. the defining test: skipping equals computing ----------------------------------------------------------------------------------
def _five_tables():
    """caller's order; engine order is requests 0, 2, 1, 4, 3 (8, 8, 5, 5, 3 levels)"""
    g = FIVE["class_guidance"]
    return [_tab(3.5, [1, 1, 0, 1, 0, 0, 1, 0]), _tab(g[1], [1, 1, 0, 1, 1]), _tab(g[2], [1, 0, 0, 0, 1, 0, 0, 1]), _tab(g[3], [1, 1, 0]),
            _tab(g[4], [1, 0, 0, 0, 0])]


def _three_tables():
    """caller's order; engine order is requests 1, 2, 0 (6, 6, 4 levels)"""
    g = BIG3["class_guidance"]
    return [_tab(g[0], [1, 1, 0, 0]), _tab(g[1], [1, 1, 0, 1, 0, 1]), _tab(g[2], [1, 0, 0, 0, 1, 0])]


def _two_tables():
    """caller's order; engine order is requests 1, 0 (6, 4 levels)"""
    g = BIG3["class_guidance"]
    return [_tab(g[0], [1, 1, 0, 0]), _tab(g[1], [0, 1, 0, 1, 0, 1])]


def _check_plan_properties(n_iter, tables, B):
    n, U, slots, widest = _plan(n_iter, tables)
    from transformer_latent_diffusion_amd import schedule
    prefix = schedule.active_prefix(sorted(n_iter, reverse=True))
    assert any(u == 0 for u in U) and any(u == b for u, b in zip(U, prefix)) and any((u + b) % 2 for u, b in zip(U, prefix))
    nonprefix = any(any(s[k] < 0 and any(v >= 0 for v in s[k + 1:]) for k in range(len(s))) for s in slots)
    assert nonprefix, "no step whose unconditional subset skips a request between two guided ones"
    finals = [float(t[-1]) for t in tables]
    assert any(f == 1.0 for f in finals) and any(f != 1.0 for f in finals)
    return n, U, widest


def _hold_skip_equals_compute(fixture, kw, tables, neg, tag, **engine):
    B = len(tables)
    n, U, widest = _check_plan_properties(kw["n_iter"], tables, B)
    m, gen = _model(fixture, **engine)
    m0, gen0 = _model(fixture, skip=False, **engine)
    eps, z0, labels = _inputs(B, seed=83)
    call = dict(seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, guidance_schedule=tables, negative_labels=neg, **_kw(kw))
    got = gen.generate_latents_requests(labels, **call)
    rows = m.sample_rows()
    want = gen0.generate_latents_requests(labels, **call)
    rows0 = m0.sample_rows()
    print(f"{tag}: {B} requests, levels {kw['n_iter']}, U per step {U}: sample rows {rows} (planner ({n}, {sum(U)})), under TLD_GUIDANCE_SKIP=0 {rows0}; "
          f"widest step {widest} samples against {2 * B}")
    assert torch.isfinite(got[0]).all()
    _equal3(got, want, f"{tag}: the skipping engine against the computing one")
    assert rows == (n, sum(U)) and rows0 == (n, n)
    return got


def test_skipping_equals_computing_tiny_five_requests():
    """one DDIM request (2), one negative label (request 1, whose unconditional sample is compacted past an unguided neighbour)"""
    eps, z0, labels = _inputs(5, seed=84)
    got = _hold_skip_equals_compute(TINY, FIVE, _five_tables(), [None, labels[0] * 0.5, None, None, None], "tiny")
    # ... and the tables are read: the result differs from the constant-guidance call
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(5, seed=83)
    const = gen.generate_latents_requests(labels, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, **FIVE)
    assert not torch.equal(got[0][1], const[1])


def test_skipping_equals_computing_100m_three_requests():
    eps, z0, labels = _inputs(3, seed=85)
    _hold_skip_equals_compute(BIG, BIG3, _three_tables(), [labels[1] * -0.5, None, None], "100m")


@pytest.mark.parametrize("cls,B", [(1, 3), (2, 2)], ids=["class1", "class2"])
def test_skipping_equals_computing_low_latency_classes(cls, B):
    kw = {k: v[:B] for k, v in BIG3.items()}
    tables = _three_tables() if B == 3 else _two_tables()
    _hold_skip_equals_compute(BIG, kw, tables, None, f"100m low-latency class {cls}", low_latency=cls, reserve=2 * B)


def test_skipping_equals_computing_without_layer0_sharing():
    """TLD_SHARE_L0=0: every model sample runs its own patch embedding, which reads the latent of its source row"""
    eps, z0, labels = _inputs(5, seed=84)
    got = _hold_skip_equals_compute(TINY, FIVE, _five_tables(), [None, labels[0] * 0.5, None, None, None], "tiny, TLD_SHARE_L0=0", share=False)
    want = _hold_skip_equals_compute(TINY, FIVE, _five_tables(), [None, labels[0] * 0.5, None, None, None], "tiny, sharing on")
    _equal3(got, want, "layer-0 sharing off against on")


def test_skipping_equals_computing_mx_fp8():
    """MX-fp8 GEMM mode at 256 tokens: equality is between the two fp8 engines"""
    _hold_skip_equals_compute(BIG, BIG3, _three_tables(), None, "100m MX-fp8", fp8=True)


# ---- 4. prefix property -------------------------------------------------------------------------------------------------------------
def test_prefix_of_a_guided_trajectory_is_the_constant_guidance_one():
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(1, seed=86)
    n, k, g = 8, 3, 4.5
    kw = dict(n_iter=n, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True)
    solo = gen.generate_latents(labels, num_imgs=1, class_guidance=g, **kw)
    got = gen.generate_latents_requests(labels, class_guidance=g, guidance_schedule=[_tab(g, [1] * k + [0] * (n - k))], **kw)
    assert torch.equal(got[1][:k], solo[1][:k]) and torch.equal(got[2][:k], solo[2][:k]), "the first k forwards differ from the constant-g call"
    assert not torch.equal(got[1][k], solo[1][k]) and not torch.equal(got[0], solo[0])
    assert m.sample_rows() == (n, k)


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------
def test_a_request_does_not_depend_on_its_neighbours():
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(5, seed=87)
    tables = _five_tables()
    neg = [None, labels[0] * 0.5, None, None, None]
    base = dict(img_size=32, sharp_f=0.1, bright_f=0.1, trace=True)
    first = gen.generate_latents_requests(labels, seeds=eps, guidance_schedule=tables, negative_labels=neg, **base, **_kw(FIVE))
    for b in range(5):                                            # alone
        s = slice(b, b + 1)
        one = gen.generate_latents_requests(labels[s], seeds=eps[s], guidance_schedule=[tables[b]], negative_labels=[neg[b]], **base,
                                            **{k: [v[b]] for k, v in _kw(FIVE).items()})
        nb = FIVE["n_iter"][b] - 1
        assert torch.equal(first[0][b], one[0][0]) and torch.equal(first[1][:nb, b], one[1][:, 0]) and torch.equal(first[2][:nb, b], one[2][:, 0]), \
            f"request {b} differs from the request alone"
        assert not first[1][nb:, b].any() and not first[2][nb:, b].any()
    perm = [3, 0, 4, 2, 1]                                        # under a permutation of the call
    second = gen.generate_latents_requests(labels[perm], seeds=eps[perm], guidance_schedule=[tables[i] for i in perm],
                                           negative_labels=[neg[i] for i in perm], **base, **{k: [v[i] for i in perm] for k, v in _kw(FIVE).items()})
    for u, v in zip(first, second):
        idx = (slice(None), perm) if u.dim() == 5 else (perm,)
        assert torch.equal(u[idx], v), "a request's result depends on the order of submission"
    other = [t.copy() for t in tables]                            # a neighbour's table changes: request 2 guided throughout, request 4 never
    other[2][:] = 2.0
    other[4][:] = 1.0
    third = gen.generate_latents_requests(labels, seeds=eps, guidance_schedule=other, negative_labels=neg, **base, **_kw(FIVE))
    for b in (0, 1, 3):
        for u, v in zip(first, third):
            assert torch.equal(u[:, b] if u.dim() == 5 else u[b], v[:, b] if v.dim() == 5 else v[b]), f"request {b} moved with a neighbour's table"
    assert not torch.equal(first[0][2], third[0][2])


# ---- 6. image-to-image and masks --------------------------------------------------------------------------------------------------------
def test_image_to_image_and_masks_in_a_guided_call():
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(3, seed=88)
    strength, masks, init = [None, 0.65, 0.65], [None, None, _rect_mask()], [None, z0[1], z0[2]]
    # 8 levels, and 5 remaining ones at strength 0.65; request 1 is unguided on its final step, request 2 guided
    tables = [_tab(3.0, [1, 0, 1, 1, 0, 0, 1, 1]), _tab(3.0, [1, 1, 0, 1, 0]), _tab(3.0, [0, 1, 0, 0, 1])]
    for sharp in (0.1, 0.0):
        kw = dict(n_iter=8, sharp_f=sharp, bright_f=sharp, trace=True)
        lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, init_latents=init, strength=strength, mask=masks, guidance_schedule=tables, **kw)
        for b in range(3):
            s = slice(b, b + 1)
            a = gen.generate_latents_requests(labels[s], seeds=eps[s], init_latents=None if init[b] is None else [init[b]], strength=[strength[b]],
                                              mask=None if masks[b] is None else [masks[b]], guidance_schedule=[tables[b]], **kw)
            n = len(tables[b]) - 1
            assert a[1].shape[0] == n
            assert torch.equal(lat[b], a[0][0]) and torch.equal(tx0[:n, b], a[1][:, 0]) and torch.equal(txt[:n, b], a[2][:, 0]), \
                f"request {b} (strength {strength[b]}, {'mask' if masks[b] is not None else 'no mask'}) differs from its solo guided call"
    keep = (masks[2] == 0).expand(4, 32, 32)                      # (the call without the latent shifts)
    assert keep.any() and torch.equal(lat[2].cpu()[keep], z0[2][keep]), "the kept region is not the initial latent"
    assert not torch.equal(lat[2].cpu()[~keep], z0[2][~keep])


# ---- 7. against the CPU reference loop ----------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def test_interval_trajectory_vs_reference_loop():
    """Tiny, 8 / 5 levels, guidance 3.0 / 4.5 at the noise levels inside [0.3, 1.0] only (so that forward 0 is the first combined
    prediction, the one the forward tolerance is stated for), real negative labels, against tests/guided_ref.py: the contract tolerances
    (the figures are printed)."""
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import schedule
    m, gen = _model(TINY)
    cfg, sd = _CACHE[(TINY, 0, True, True, False)][2:]
    eps, z0, labels = _inputs(2, seed=89)
    neg = torch.randn(2, 768, generator=torch.Generator().manual_seed(90)) * 0.5
    n_iter, g, iv = [8, 5], [3.0, 4.5], (0.3, 1.0)
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, n_iter=n_iter, class_guidance=g, negative_labels=neg, sharp_f=0.1, bright_f=0.1,
                                                  trace=True, guidance_interval=iv)
    levels = [schedule.noise_schedule(n, 1) for n in n_iter]
    tables = [schedule.guidance_table(schedule.step_coefficients(lv), gb, iv) for lv, gb in zip(levels, g)]
    assert all(1.0 in t.tolist() and t[0] == np.float32(gb) and t[-1] == 1.0 for t, gb in zip(tables, g))
    n, U, _, _ = _plan(n_iter, tables)
    assert m.sample_rows() == (n, sum(U)) and sum(U) < n
    ref = TorchRefDenoiser(asdict(cfg), sd)
    rlat, rx0, rxt = G.sample_requests(ref, eps, None, None, labels, [neg[0], neg[1]], levels, [1.0, 1.0], tables, [True, True], 0.1, 0.1, trace=True)
    lat, tx0, txt = lat.cpu(), tx0.cpu(), txt.cpu()
    for b in range(2):
        k = n_iter[b] - 1
        e_first = _rel_rms(tx0[0, b], rx0[0, b])                              # the first combined prediction
        e_lat = _rel_rms(lat[b], rlat[b])
        e_x0 = max(_rel_rms(tx0[i, b], rx0[i, b]) for i in range(k))
        e_xt = max(_rel_rms(txt[i, b], rxt[i, b]) for i in range(k))
        print(f"interval trajectory request {b} (g {g[b]} in {iv}, table {tables[b].tolist()}): first combined prediction {e_first:.3e}, end latent "
              f"{e_lat:.3e}, worst-step trace_x0 {e_x0:.3e}, trace_xt {e_xt:.3e}")
        assert np.isfinite(e_first) and e_first <= FWD_TOL
        for e in (e_lat, e_x0, e_xt):
            assert np.isfinite(e) and e <= TRAJ_TOL


# ---- 8. the surface ---------------------------------------------------------------------------------------------------------------------
def test_generate_latents_with_an_interval_and_repeatability():
    m, gen = _model(TINY)
    eps, z0, labels = _inputs(4, seed=91)
    kw = dict(n_iter=8, class_guidance=3.0, img_size=32, sharp_f=0.1, bright_f=0.1, seeds=eps, trace=True)
    before = gen.generate_latents(labels, num_imgs=4, **kw)
    got = gen.generate_latents(labels, num_imgs=4, guidance_interval=(0.3, 0.8), **kw)
    rows = m.sample_rows()
    want = gen.generate_latents_requests(labels, guidance_interval=[(0.3, 0.8)] * 4, **kw)
    _equal3(got, want, "generate_latents with an interval against generate_latents_requests")
    assert rows == m.sample_rows() and rows[1] < rows[0] == 32 and not torch.equal(got[0], before[0])
    frm = gen.generate_latents_from(z0, labels, strength=0.65, guidance_interval=(0.3, 0.8), **{k: v for k, v in kw.items() if k != "img_size"})
    frm_r = gen.generate_latents_requests(labels, init_latents=z0, strength=0.65, guidance_interval=(0.3, 0.8), **kw)
    _equal3(frm, frm_r, "generate_latents_from with an interval against generate_latents_requests")
    # one update launch per step
    m.set_profile(["update"])
    try:
        gen.generate_latents_requests(labels, guidance_interval=(0.3, 0.8), **dict(kw, n_iter=[8, 5, 6, 3]))
        ms, n = m.get_profile("update")
    finally:
        m.set_profile([])
    assert n == 8 and ms > 0.0, (n, ms)
    # the launch paths are those of the requests step, and a plain call afterwards is what it was before
    from transformer_latent_diffusion_amd import Denoiser
    m.set_debug(True)
    try:
        gen.generate_latents_requests(labels, guidance_interval=(0.3, 0.8), **kw)
        paths = m.debug_paths()
    finally:
        m.set_debug(False)
    assert (paths >> 50) == 1 << (58 - 50), f"sampler path bits {paths >> 50:#x}"
    after = gen.generate_latents(labels, num_imgs=4, **kw)
    _equal3(after, before, "a plain generate_latents after guided calls")
    assert m.sample_rows() == (32, 32)


def test_device_side_refusal_enqueues_nothing():
    from transformer_latent_diffusion_amd import _lib, schedule
    m, gen = _model(TINY)
    cap = m._engine_batch
    dev = _dev()
    B = cap // 2 + 1                                              # B <= cap < 2 B
    co = schedule.step_coefficients(schedule.noise_schedule(4, 1))
    tab = np.tile(co, (B, 1, 1))
    recs = (_lib.TldSampleRequest * B)(*[_lib.TldSampleRequest(4, 0.0, 1.0, 0)] * B)
    x = torch.zeros(B, 4, 32, 32, device=dev)
    lab = torch.zeros(B, 768, device=dev)
    sentinel = torch.full_like(x, 7.0)
    L = _lib.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(g):
        rc = L.tld_sample_requests_guided(m._engine, C.c_void_p(x.data_ptr()), None, None, C.c_void_p(lab.data_ptr()), None, recs, fp(tab), fp(g), 4, 0.0,
                                          0.0, C.c_void_p(sentinel.data_ptr()), B, None, None, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        return rc, L.tld_last_error().decode()

    g = np.ones((B, 4), dtype=np.float32)
    g[:, 2] = 3.0                                                 # step 2 runs B + B samples
    rc, msg = call(g)
    assert rc == 1 and "max_batch" in msg and "step 2" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()), "a refused call wrote its output"
    g[cap - B:, 2] = 1.0                                          # B + (cap - B) samples: it fits
    rc, msg = call(g)
    torch.cuda.synchronize()
    assert rc == 0 and not bool((sentinel == 7.0).any()), (rc, msg)
    assert m.sample_rows() == (4 * B, cap - B)


def test_pipeline_and_mixed_batcher_take_an_interval():
    from PIL import Image
    from transformer_latent_diffusion_amd import (AutoencoderKLDecoder, DenoiserConfig, DiffusionTransformer, LTDConfig, RequestBatcher,
                                                  VaeDecoderConfig)
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(_dev())
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2).to(_dev())

    class Tok:                                                    # clip.tokenize stand-in: SOT, one id per character, EOT, zero padding
        def tokenize(self, prompts, truncate=True):
            t = torch.zeros(len(prompts), ccfg.context_length, dtype=torch.long)
            for i, p in enumerate(prompts):
                ids = [1 + (ord(ch) % 900) for ch in p][: ccfg.context_length - 2]
                t[i, 0] = ccfg.vocab_size - 2
                t[i, 1:1 + len(ids)] = torch.tensor(ids)
                t[i, 1 + len(ids)] = ccfg.vocab_size - 1
            return t

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=vae, clip_model=enc, tokenizer=Tok(), run_device=_dev())
    prompts, guid, n_it, seeds = ["a cute cat", "a red car", "a tall tree"], [6.0, 3.0, 4.5], [4, 6, 5], [3, 4, 5]
    ivs = [(0.3, 0.8), None, (0.0, 0.5)]
    plain = pipe.generate_images_from_texts(prompts, class_guidance=guid, seeds=seeds, n_iter=n_it)
    pics = pipe.generate_images_from_texts(prompts, class_guidance=guid, seeds=seeds, n_iter=n_it, guidance_interval=ivs)
    rows = pipe.diffuser.model.sample_rows()
    assert len(pics) == 3 and all(isinstance(p, Image.Image) for p in pics)
    assert rows[0] == sum(n_it) and 0 < rows[1] < rows[0]
    assert np.array_equal(np.asarray(pics[1]), np.asarray(plain[1])) and not np.array_equal(np.asarray(pics[0]), np.asarray(plain[0]))
    for i in (0, 2):
        alone = pipe.generate_image_from_text(prompts[i], class_guidance=guid[i], seed=seeds[i], n_iter=n_it[i], guidance_interval=ivs[i])
        assert np.array_equal(np.asarray(pics[i]), np.asarray(alone)), f"prompt {i}: the batched picture differs from the one-prompt call"
    rb = RequestBatcher(pipe, max_batch=8, mixed=True)
    tickets = [rb.submit(p, g, s, n, guidance_interval=iv) for p, g, s, n, iv in zip(prompts, guid, seeds, n_it, ivs)]
    res = rb.flush()
    for t, p in zip(tickets, pics):
        assert np.array_equal(np.asarray(res[t]), np.asarray(p)), "the mixed batcher's picture differs"

"""GPU: guidance rescale and adaptive projected guidance inside the sampler's step (tld_sample_requests_shaped).

The statistics kernel and the combine alone, through tld_debug_guidance_shape: the five double sums against math.fsum, (P, Q) against the host
finalisation on the DEVICE's sums, x0 bit for bit against numpy with the device's (P, Q), the momentum chained over two calls, independence of the
batch, and the two defining properties on the device's x0.  Then the sampler: neutral rows are the older entries bit for bit; the first shaped
forward of a call is the debug entry's x0 on that forward's (cond, unc), at V = 4 and V = 1, with and without a mask; a request of a mixed call is
the request alone; the trajectories meet the contract tolerances against tests/shaped_ref.py; the pipeline, the batcher, the accounting and the
refusals.  Engine shapes: d = 128, 2 layers, 16 x 16 latents (img 1024) and 24 x 24 (img 2304).  Every test prints the figures it asserts."""
import ctypes as C
import math
from dataclasses import asdict

import numpy as np
import pytest
import torch

import shaped_ref as R

pytestmark = pytest.mark.gpu

TRAJ_TOL = 6e-2          # the contract tolerance of a multi-step CFG trajectory (tests/test_gpu_parity.py)
FWD_TOL = 2e-2           # ... of one forward
IMGS = (4, 6, 1020, 1024, 1028, 2304, 65536)
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(size=16, low_latency=0):
    key = (size, low_latency)
    if key not in _CACHE:
        from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator
        from transformer_latent_diffusion_amd.weights import synth_state_dict
        cfg = DenoiserConfig(image_size=size, patch_size=2, embed_dim=128, n_layers=2, n_channels=4)
        sd = synth_state_dict(cfg, 7)
        m = Denoiser(**asdict(cfg)).to(_dev())
        if low_latency:
            m.set_low_latency(low_latency)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        _CACHE[key] = (cfg, sd, m, DiffusionGenerator(m, None, _dev(), torch.float32))
    return _CACHE[key]


def _inputs(B, S_=16, seed=201):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S_, S_, generator=gen)
    z0 = torch.randn(B, 4, S_, S_, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


def _rect_mask(S_=16):
    m = torch.zeros(1, S_, S_)
    m[:, 3:11, 2:9] = 1
    return m


def _cu(batch, n, seed):
    """c with mean 0.3, u = 0.8 c + 0.4 noise, and a momentum buffer like an earlier update: float32 [batch, n]"""
    rng = np.random.default_rng(seed)
    c = (rng.standard_normal((batch, n)) + 0.3).astype(np.float32)
    u = (np.float32(0.8) * c + np.float32(0.4) * rng.standard_normal((batch, n)).astype(np.float32)).astype(np.float32)
    m = (np.float32(0.2) * c + np.float32(0.4) * rng.standard_normal((batch, n)).astype(np.float32)).astype(np.float32)
    return c, u, m


def _debug(c, u, m, g, rows):
    """tld_debug_guidance_shape on host arrays [batch, img] (m None: no buffer) -> x0, pq [batch, 2], sums [batch, 5], the buffer afterwards"""
    from transformer_latent_diffusion_amd import _lib
    dev = _dev()
    t = lambda a: None if a is None else (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).to(dev).contiguous()
    ct, ut, mt = t(c), t(u), t(m)
    batch, img = ct.shape[0], ct[0].numel()
    x0, pq, sums = torch.empty_like(ct), torch.empty(batch, 2, device=dev), torch.empty(batch, 5, device=dev, dtype=torch.float64)
    garr, sarr = np.ascontiguousarray(g, dtype=np.float32), np.ascontiguousarray(rows, dtype=np.float32).reshape(batch, 4)
    vp = lambda a: C.c_void_p(None if a is None else a.data_ptr())
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    _lib.check(_lib.lib().tld_debug_guidance_shape(vp(ct), vp(ut), vp(mt), fp(garr), fp(sarr), batch, img, vp(x0), vp(pq), vp(sums),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_debug_guidance_shape")
    torch.cuda.synchronize()
    return x0.cpu().numpy(), pq.cpu().numpy(), sums.cpu().numpy(), None if mt is None else mt.cpu().numpy()


def _adjacent(a, b):
    a, b = np.float32(a), np.float32(b)
    return a == b or np.nextafter(a, b) == b


ROWS3 = [(1.0, 0.0, 0.0, 1.0), (0.0, 2.5, -0.5, 0.0), (0.5, 0.0, -0.75, 0.7)]
G3 = [6.0, 4.5, 7.5]


# ---- 1. the statistics kernel and the combine alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("img", IMGS)
def test_debug_entry_sums_weights_and_x0(img):
    """Sums: |device - fsum| <= 1e-12 sum |terms| (a thread adds at most 256 values of one sign pattern and the tree has 8 levels: the bound of a
    recursive sum of 264 roundings at 2^-53 is 3e-14 sum |terms|).  (P, Q): equal or adjacent to the host finalisation on the device's sums (libm
    and the device's sqrt and division may differ in the last bit of a double, which the fp32 rounding shows at most as a neighbour).  x0: bit for
    bit fl32(fma(P, c, fl32(Q dbar))) with the device's P, Q.  The momentum: two chained calls; an entry alone."""
    c, u, m = _cu(3, img, 400 + img)
    x0, pq, sums, m1 = _debug(c, u, m, G3, ROWS3)
    worst = 0.0
    for b in range(3):
        db = R.dbar_f32(c[b], u[b], m[b], ROWS3[b][2])
        want, scale = R.sums_f64(c[b], db), R.abs_sums_f64(c[b], db)
        for j in range(5):
            err = abs(sums[b, j] - want[j]) / scale[j]
            worst = max(worst, err)
            assert err <= 1e-12, (img, b, j, sums[b, j], want[j])
        P, Q = R.finalize(sums[b], img, G3[b], ROWS3[b])
        assert _adjacent(pq[b, 0], P) and _adjacent(pq[b, 1], Q), (img, b, pq[b], P, Q)
        assert np.array_equal(x0[b], R.fma_f32(pq[b, 0], c[b], pq[b, 1] * db)), (img, b)
        # the buffer: dbar where beta != 0, untouched elsewhere
        assert np.array_equal(m1[b], db if ROWS3[b][2] != 0 else m[b]), (img, b)
    # chained: the second call's dbar is fl32(d + fl32(beta dbar_1)), bit for bit
    c2, u2, _ = _cu(3, img, 500 + img)
    x02, pq2, sums2, m2 = _debug(c2, u2, m1, G3, ROWS3)
    for b in range(3):
        db2 = R.dbar_f32(c2[b], u2[b], m1[b], ROWS3[b][2])
        assert np.array_equal(m2[b], db2 if ROWS3[b][2] != 0 else m1[b])
        assert np.array_equal(x02[b], R.fma_f32(pq2[b, 0], c2[b], pq2[b, 1] * db2))
    # an entry does not depend on the others or on the batch
    for b, order in ((1, [1]), (2, [2, 0])):
        xa, pa, sa, ma = _debug(c[order], u[order], m[order], [G3[i] for i in order], [ROWS3[i] for i in order])
        assert np.array_equal(xa[0], x0[b]) and np.array_equal(pa[0], pq[b]) and np.array_equal(sa[0], sums[b]) and np.array_equal(ma[0], m1[b])
    # a neutral row: plain CFG, zeros in the tables; without the buffer beta must be 0
    xn, pn, sn, _ = _debug(c[:1], u[:1], None, [6.0], [R.NEUTRAL])
    assert np.array_equal(xn[0], R.fma_f32(np.float32(6.0), c[0], np.float32(-5.0) * u[0])) and not pn.any() and not sn.any()
    print(f"img {img}: sums within {worst:.2e} of sum |terms|; (P, Q) {pq.tolist()}")


@pytest.mark.parametrize("img", IMGS)
def test_debug_entry_properties(img):
    """On the device's x0, bound 1e-5 (fp32 P, Q and products over up to 65536 terms): phi = 1 gives std(x0) = std(c); eta_par = 0 without clip and
    momentum gives <x0 - c, c> = 0, relative to |x0 - c| |c|.  Inputs with |A| > 1e-3 in the statement, checked here on the CPU."""
    c, u, m = _cu(3, img, 600 + img)
    rows = [(1.0, 0.0, 0.0, 1.0), (0.3, 3.0, -0.5, 1.0), (0.0, 0.0, 0.0, 1.0)]
    gs = [6.0, 4.0, 7.0]
    for b in range(3):
        db = R.dbar_f32(c[b], u[b], m[b], rows[b][2])
        assert abs(R.weights_AB(R.sums_f64(c[b], db), gs[b], rows[b])[0]) > 1e-3
    x0 = _debug(c, u, m, gs, rows)[0].astype(np.float64)
    e_std = max(abs(x0[b].std() - c[b].astype(np.float64).std()) / c[b].astype(np.float64).std() for b in range(3))
    rows = [(0.0, 0.0, 0.0, 0.0)] * 3
    gs = [6.0, 1.5, 0.0]
    for b in range(3):
        assert abs(R.weights_AB(R.sums_f64(c[b], R.dbar_f32(c[b], u[b], None, 0.0)), gs[b], rows[b])[0]) > 1e-3
    x0 = _debug(c, u, None, gs, rows)[0].astype(np.float64)
    c64 = c.astype(np.float64)
    e_dot = max(abs(np.dot(x0[b] - c64[b], c64[b])) / (np.linalg.norm(x0[b] - c64[b]) * np.linalg.norm(c64[b])) for b in range(3))
    print(f"img {img}: |std(x0) - std(c)| / std(c) {e_std:.2e}; |<x0 - c, c>| / (|x0 - c| |c|) {e_dot:.2e}")
    assert e_std <= 1e-5 and e_dot <= 1e-5


@pytest.mark.parametrize("img", [1024, 2304])
def test_debug_entry_on_unaligned_operands_and_at_guidance_one(img):
    """cond / unc / the momentum buffer as views that start 4 bytes into their buffers, img a multiple of 4: the scalar flavour of the statistics
    kernel, bit for bit the 16-byte one's sums, weights, x0 and buffer.  And an entry guided at exactly 1.0 is unguided whatever its row says:
    x0 = fma(1, c, 0 u), nothing in the tables, the momentum buffer left alone."""
    from transformer_latent_diffusion_amd import _lib
    dev = _dev()
    c, u, m = _cu(3, img, 700 + img)
    want = _debug(c, u, m, G3, ROWS3)
    bufs = [torch.zeros(3 * img + 4, device=dev) for _ in range(3)]
    views = [b[1:1 + 3 * img].view(3, img) for b in bufs]
    for v, a in zip(views, (c, u, m)):
        v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4
    x0, pq, sums = torch.empty(3, img, device=dev), torch.empty(3, 2, device=dev), torch.empty(3, 5, device=dev, dtype=torch.float64)
    garr, sarr = np.array(G3, np.float32), np.ascontiguousarray(ROWS3, dtype=np.float32)
    vp = lambda a: C.c_void_p(a.data_ptr())
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    _lib.check(_lib.lib().tld_debug_guidance_shape(vp(views[0]), vp(views[1]), vp(views[2]), fp(garr), fp(sarr), 3, img, vp(x0), vp(pq), vp(sums),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_debug_guidance_shape")
    torch.cuda.synchronize()
    assert np.array_equal(x0.cpu().numpy(), want[0]) and np.array_equal(pq.cpu().numpy(), want[1]) and np.array_equal(sums.cpu().numpy(), want[2])
    assert np.array_equal(views[2].cpu().numpy(), want[3])
    assert all(float(b[0]) == 0.0 and float(b[-3:].abs().max()) == 0.0 for b in bufs)
    xg, pg, sg, mg = _debug(c, u, m, [1.0, 6.0, 1.0], ROWS3)
    for b in (0, 2):
        assert np.array_equal(xg[b], R.fma_f32(np.float32(1.0), c[b], np.float32(0.0) * u[b])) and np.array_equal(xg[b], c[b])
        assert not pg[b].any() and not sg[b].any() and np.array_equal(mg[b], m[b])
    assert pg[1].any() and not np.array_equal(mg[1], m[1])


# ---- 2. neutral rows through the new entry ----------------------------------------------------------------------------------------------------------------
def _equal3(a, b, what):
    for u, v, name in zip(a, b, ("end latent", "trace_x0", "trace_xt")):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {name} differs"


def test_neutral_rows_are_the_older_entries_bit_for_bit():
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model()
    B = 4
    eps, z0, labels = (t.to(_dev()) for t in _inputs(B))
    n_iter, guid, plus = [6, 4, 6, 3], [3.0, 4.5, 1.0, 6.0], [True, True, False, True]
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1), p) for n, p in zip(n_iter, plus)]
    neutral = [R.NEUTRAL] * B
    common = dict(sharp_f=0.1, bright_f=0.1, trace=True)
    # (a) the stochastic entry at eta > 0, on a guidance table with skipped steps, masked
    sde = [schedule.step_coefficients(schedule.noise_schedule(n, 1), p, eta=1.0) for n, p in zip(n_iter, plus)]
    tables = [np.array([3.0, 3.0, 1.0, 1.0, 3.0, 1.0], np.float32), np.array([1.0, 4.5, 4.5, 1.0], np.float32), np.ones(6, np.float32),
              np.array([6.0, 1.0, 6.0], np.float32)]
    mask = torch.stack([_rect_mask()] * B).to(_dev())
    kw = dict(guidance_steps=tables, noise_coeffs=[e for _, e in sde], noise_keys=[11, 12, 13, 14], init_latents=z0, mask=mask, **common)
    want = m.sample_latents_requests(eps, labels, [co for co, _ in sde], None, **kw)
    rows_want = m.sample_rows()
    got = m.sample_latents_requests(eps, labels, [co for co, _ in sde], None, shape=neutral, **kw)
    _equal3(got, want, "neutral rows beside tld_sample_requests_stochastic (eta 1, masked, guidance table)")
    assert m.sample_rows() == rows_want and rows_want[1] < rows_want[0]
    # (b) the guided entry (noise NULL)
    want = m.sample_latents_requests(eps, labels, coeffs, None, guidance_steps=tables, **common)
    got = m.sample_latents_requests(eps, labels, coeffs, None, guidance_steps=tables, shape=neutral, **common)
    _equal3(got, want, "neutral rows beside tld_sample_requests_guided")
    # (c) the plain entry (noise and guidance NULL), masked
    want = m.sample_latents_requests(eps, labels, coeffs, guid, init_latents=z0, mask=mask, **common)
    got = m.sample_latents_requests(eps, labels, coeffs, guid, init_latents=z0, mask=mask, shape=neutral, **common)
    _equal3(got, want, "neutral rows beside tld_sample_requests (masked)")
    assert m.sample_rows() == (sum(n_iter), sum(n_iter))
    # request 2 is guided at exactly 1.0 and, without a table, still runs its unconditional sample: a shape on it changes nothing, momentum included
    rows = [R.NEUTRAL, R.NEUTRAL, (0.0, 2.5, -0.5, 0.7), R.NEUTRAL]
    got = m.sample_latents_requests(eps, labels, coeffs, guid, init_latents=z0, mask=mask, shape=rows, **common)
    _equal3(got, want, "a shaped request guided at 1.0 on the CFG-doubled batch")
    # (d) generate_latents: a uniform batch; and one shaped request in the call leaves the neutral ones alone
    kw = dict(n_iter=6, class_guidance=3.0, img_size=16, sharp_f=0.1, bright_f=0.1, seeds=eps, trace=True)
    want = gen.generate_latents(labels, num_imgs=B, **kw)
    co = schedule.step_coefficients(schedule.noise_schedule(6, 1))
    got = m.sample_latents_requests(eps, labels, [co] * B, [3.0] * B, shape=neutral, **common)
    _equal3(got, want, "neutral rows beside generate_latents")
    one = m.sample_latents_requests(eps, labels, [co] * B, [3.0] * B, shape=[R.NEUTRAL, (0.0, 2.5, -0.5, 0.7), R.NEUTRAL, R.NEUTRAL], **common)
    assert [torch.equal(one[0][b], want[0][b]) for b in range(B)] == [True, False, True, True]
    print("neutral rows: bitwise equal to the stochastic (eta 1, masked), the guided, the plain entry and generate_latents")


# ---- 3. the first shaped forward inside the sampler, exactly --------------------------------------------------------------------------------------------
def _direct(m, eps, labels, coeffs, gtab, rows, out, tx0, txt, z0=None, mask=None):
    """tld_sample_requests_shaped straight through ctypes on the caller's device tensors (equal level counts, no noise, a guidance table)"""
    from transformer_latent_diffusion_amd import _lib
    B, n_max = eps.shape[0], coeffs.shape[0]
    table = np.ascontiguousarray(np.tile(coeffs, (B, 1, 1)), dtype=np.float32)
    recs = (_lib.TldSampleRequest * B)(*[_lib.TldSampleRequest(n_max, 1.0, 1.0, 0) for _ in range(B)])
    g = np.ascontiguousarray(gtab, dtype=np.float32).reshape(B, n_max)
    s = np.ascontiguousarray(rows, dtype=np.float32).reshape(B, 4)
    h = m._ensure_engine(2 * B, _dev())
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = _lib.lib().tld_sample_requests_shaped(h, vp(eps), vp(z0), vp(mask), vp(labels), None, recs, fp(table), fp(g), None, None, fp(s), n_max, 0.1, 0.1,
                                               vp(out), B, vp(tx0), vp(txt), C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))
    assert rc == 0, _lib.lib().tld_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("size", [16, 24])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_first_shaped_forward_is_the_debug_entry_on_that_forward(size, masked):
    """Guidance 1.0 at a forward leaves trace_x0 = cond (no unconditional sample runs), guidance 0.0 leaves fma(0, c, u) = unc: two guided calls give the
    (cond, unc) of forward 0, and, unguided at forward 0, two more give those of forward 1.  The shaped call's trace_x0 there equals
    tld_debug_guidance_shape on that pair -- at forward 1 with a zero momentum buffer, because the unguided forward 0 did not touch it.  V = 4, and V = 1
    through out_latent / trace_xt views that start 4 bytes into their buffers; trace_x0 is the unblended prediction, so the mask changes nothing here."""
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(size)
    dev = _dev()
    B, n = 2, 4
    eps, z0, labels = (t.to(dev).contiguous() for t in _inputs(B, size, seed=203 + size))
    mask = torch.stack([_rect_mask(size), 1 - _rect_mask(size)]).to(dev).contiguous() if masked else None
    co = schedule.step_coefficients(schedule.noise_schedule(n, 1))
    rows, g = [(0.0, 2.5, -0.5, 0.7), (1.0, 0.0, 0.0, 1.0)], [6.0, 3.0]
    numel = eps.numel()
    img = numel // B

    def run(gtab, shape_rows, odd=False):
        out, tx0 = torch.empty_like(eps), torch.zeros((n - 1,) + tuple(eps.shape), device=dev)
        if not odd:
            txt = torch.zeros_like(tx0)
            _direct(m, eps, labels, co, gtab, shape_rows, out, tx0, txt, z0 if masked else None, mask)
            return out, tx0, txt
        buf_o, buf_t = torch.zeros(numel + 4, device=dev), torch.zeros((n - 1) * numel + 4, device=dev)
        out_u, txt_u = buf_o[1:1 + numel].view_as(eps), buf_t[1:1 + (n - 1) * numel].view(n - 1, *eps.shape)
        assert out_u.data_ptr() % 16 == 4 and txt_u.data_ptr() % 16 == 4
        _direct(m, eps, labels, co, gtab, shape_rows, out_u, tx0, txt_u, z0 if masked else None, mask)
        assert float(buf_o[0]) == 0.0 and float(buf_o[-3:].abs().max()) == 0.0 and float(buf_t[0]) == 0.0 and float(buf_t[-3:].abs().max()) == 0.0
        return out_u.clone(), tx0, txt_u.clone()

    neutral = [R.NEUTRAL] * B
    tab = lambda first, second: [[first, second, gb, gb] for gb in g]
    c0 = run(tab(1.0, 1.0), neutral)[1][0]
    u0 = run(tab(0.0, 1.0), neutral)[1][0]
    c1 = run(tab(1.0, 1.0), neutral)[1][1]
    u1 = run(tab(1.0, 0.0), neutral)[1][1]
    assert not torch.equal(c0, u0) and not torch.equal(c1, u1)
    want0 = _debug(c0.reshape(B, img), u0.reshape(B, img), torch.zeros(B, img), g, rows)
    want1 = _debug(c1.reshape(B, img), u1.reshape(B, img), torch.zeros(B, img), g, rows)
    for odd in (False, True):
        first = run([[gb] * n for gb in g], rows, odd)
        assert np.array_equal(first[1][0].cpu().numpy().reshape(B, img), want0[0]), f"V = {1 if odd else 4}: forward 0 is not the debug entry's x0"
        late = run([[1.0, gb, gb, gb] for gb in g], rows, odd)
        assert torch.equal(late[1][0], c0)
        assert np.array_equal(late[1][1].cpu().numpy().reshape(B, img), want1[0]), f"V = {1 if odd else 4}: forward 1 after an unguided forward 0"
        if not odd:
            vec = (first, late)
        else:
            _equal3(first, vec[0], "the scalar instantiation beside the 16-byte one")
            _equal3(late, vec[1], "the scalar instantiation beside the 16-byte one (shaped from forward 1)")
    # the second shaped forward reads the first one's update: with beta = 0 on the same call request 0 moves from forward 1 on, request 1 (beta 0) does not
    nomom = run([[gb] * n for gb in g], [(0.0, 2.5, 0.0, 0.7), rows[1]])
    assert torch.equal(nomom[1][0], vec[0][1][0]) and not torch.equal(nomom[1][1, 0], vec[0][1][1, 0]) and torch.equal(nomom[1][:, 1], vec[0][1][:, 1])
    if masked:
        keep = (mask[0] == 0).expand(4, size, size)
        assert torch.equal(vec[0][0][0][keep], z0[0][keep] + torch.tensor([0.1, 0, 0, 0.1], device=dev).view(4, 1, 1).expand(4, size, size)[keep])
    print(f"size {size} ({'masked' if masked else 'plain'}): forward 0 and forward 1 of the shaped call equal the debug entry bit for bit at V = 4 and V = 1")


# ---- 4. a request of a mixed call is the request alone ----------------------------------------------------------------------------------------------------
MIX = dict(n_iter=[7, 5, 7, 3], class_guidance=[6.0, 4.5, 3.0, 6.0], use_ddpm_plus=[True, True, False, True], eta=[0.0, 0.0, 1.0, 0.0],
           guidance_rescale=[0.7, 0.0, 1.0, 0.0], apg_eta=[1.0, 1.0, 0.25, 0.0], apg_norm=[0.0, 0.0, 0.0, 2.5], apg_momentum=[0.0, 0.0, -0.5, -0.75],
           strength=[None, None, None, 0.8], guidance_interval=[(0.2, 0.9), None, None, None])
MIX_KEYS = [5, 6, 7 | (3 << 32), 8]


def _call_mixed(gen, eps, labels, z0, idx, size=16, kw=MIX):
    neg = [None, None, labels[0] * 0.5, None]
    mask = [None, None, None, _rect_mask(size)]
    init = [None, None, None, z0[3]]
    pick = lambda v: [v[i] for i in idx]
    return gen.generate_latents_requests(labels[idx], seeds=eps[idx], img_size=size, sharp_f=0.1, bright_f=0.1, trace=True, negative_labels=pick(neg),
                                         mask=pick(mask), init_latents=pick(init), noise_seeds=pick(MIX_KEYS), **{k: pick(v) for k, v in kw.items()})


@pytest.mark.parametrize("size", [16, 24])
def test_request_of_a_mixed_call_equals_the_request_alone_in_both_orders(size):
    """Four requests: rescale under an interval; a neutral one; rescale + APG with momentum on a negative label at eta = 1 (DDIM); APG with clip and momentum,
    masked image-to-image, fewest levels."""
    cfg, sd, m, gen = _model(size)
    eps, z0, labels = _inputs(4, size, seed=204)
    lat, tx0, txt = _call_mixed(gen, eps, labels, z0, list(range(4)), size)
    assert torch.isfinite(lat).all()
    for b in range(4):
        a, ax0, axt = _call_mixed(gen, eps, labels, z0, [b], size)
        nb = ax0.shape[0]
        assert torch.equal(lat[b], a[0]) and torch.equal(tx0[:nb, b], ax0[:, 0]) and torch.equal(txt[:nb, b], axt[:, 0]), f"request {b} differs from the request alone"
        assert not tx0[nb:, b].any() and not txt[nb:, b].any()
    perm = [3, 0, 2, 1]
    second = _call_mixed(gen, eps, labels, z0, perm, size)
    for u, v in zip((lat, tx0, txt), second):
        idx = (slice(None), perm) if u.dim() == 5 else (perm,)
        assert torch.equal(u[idx], v), "a request's result depends on the order of submission"
    # the shape is there: the same call with neutral rows differs in the shaped requests, and only there
    off = dict(MIX, guidance_rescale=[0.0] * 4, apg_eta=[1.0] * 4, apg_norm=[0.0] * 4, apg_momentum=[0.0] * 4)
    det = _call_mixed(gen, eps, labels, z0, list(range(4)), size, kw=off)
    assert [not torch.equal(lat[b], det[0][b]) for b in range(4)] == [True, False, True, True]
    print(f"mixed call at size {size}: 4 requests bitwise equal to each request alone, in either order")


def _big_low_latency():
    """The 100 M model in low-latency class 1 (the class needs embed_dim 384 or 768): the fixture of tests/test_gpu_stochastic.py"""
    if "big" not in _CACHE:
        from conftest import cfg_from_arr, load_golden, synth_weights
        from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
        g = load_golden("g5_100m.npz")
        cfg = cfg_from_arr(g["cfg"])
        sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
        m = Denoiser(**asdict(cfg)).to(_dev())
        m.set_low_latency(1)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        _CACHE["big"] = (cfg, m, DiffusionGenerator(m, None, _dev(), torch.float32))
    return _CACHE["big"]


def test_mixed_call_in_low_latency_class_1():
    cfg, m, gen = _big_low_latency()
    S_ = cfg.image_size
    eps, z0, labels = _inputs(3, S_, seed=205)
    kw = dict(n_iter=[4, 3, 4], class_guidance=[6.0, 3.0, 4.5], use_ddpm_plus=[True, True, False], guidance_rescale=[0.7, 0.0, 0.0], apg_eta=[1.0, 1.0, 0.0],
              apg_momentum=[0.0, 0.0, -0.5], img_size=S_, sharp_f=0.1, bright_f=0.1, trace=True)
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, **kw)
    for b in range(3):
        solo = gen.generate_latents_requests(labels[b:b + 1], seeds=eps[b:b + 1], **{k: ([v[b]] if isinstance(v, list) else v) for k, v in kw.items()})
        nb = solo[1].shape[0]
        assert torch.equal(lat[b], solo[0][0]) and torch.equal(txt[:nb, b], solo[2][:, 0]), f"low-latency class 1: request {b} differs from the request alone"


# ---- 5. against the CPU reference loop ----------------------------------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def _device_noise(keys, steps, img):
    from transformer_latent_diffusion_amd import _lib
    dev = _dev()
    k = torch.tensor(np.array(keys, dtype=np.uint64).view(np.int64), device=dev)
    s = torch.tensor(np.array(steps, dtype=np.uint32).view(np.int32), device=dev)
    out = torch.empty(len(keys), img, device=dev)
    _lib.check(_lib.lib().tld_debug_sampler_noise(C.c_void_p(k.data_ptr()), C.c_void_p(s.data_ptr()), len(keys), img, C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_debug_sampler_noise")
    torch.cuda.synchronize()
    return out.cpu()


@pytest.fixture(scope="module")
def torch_ref():
    from oracle.torch_ref import TorchRefDenoiser
    cfg, sd, m, gen = _model()
    return TorchRefDenoiser(asdict(cfg), sd)


@pytest.mark.parametrize("case", ["rescale", "apg", "both"])
def test_trajectory_vs_reference_loop(torch_ref, case):
    """6 levels, DPM-Solver++(2M) deterministic and DDIM at eta = 1 (fed the device's z), guidance 6.0 / 4.5, against tests/shaped_ref.py in float32: the
    contract tolerances of tests/test_gpu_parity.py for the first combined prediction and the end latent."""
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model()
    shape = {"rescale": dict(guidance_rescale=0.7), "apg": dict(apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5),
             "both": dict(guidance_rescale=0.7, apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5)}[case]
    row = schedule.check_guidance_shape(**shape)
    eps, z0, labels = _inputs(2, seed=206)
    g, plus, eta, keys, n_iter = [6.0, 4.5], [True, False], [0.0, 1.0], [31, 32 | (1 << 32)], 6
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, n_iter=n_iter, class_guidance=g, use_ddpm_plus=plus, eta=eta, noise_seeds=keys,
                                                  img_size=16, sharp_f=0.1, bright_f=0.1, trace=True, **shape)
    levels = [schedule.noise_schedule(n_iter, 1)] * 2
    z = [None, [zz.reshape(4, 16, 16) for zz in _device_noise([keys[1]] * (n_iter - 1), list(range(n_iter - 1)), 4 * 16 * 16)]]
    rlat, rx0, rxt = R.sample_requests(torch_ref, eps, None, None, labels, None, levels, [1.0, 1.0], [[g[b]] * n_iter for b in range(2)], plus, eta, z,
                                       [row, row], 0.1, 0.1, trace=True)
    plain = gen.generate_latents_requests(labels, seeds=eps, n_iter=n_iter, class_guidance=g, use_ddpm_plus=plus, eta=eta, noise_seeds=keys, img_size=16,
                                          sharp_f=0.1, bright_f=0.1)
    lat, tx0, txt = lat.cpu(), tx0.cpu(), txt.cpu()
    for b in range(2):
        e_first, e_lat = _rel_rms(tx0[0, b], rx0[0, b]), _rel_rms(lat[b], rlat[b])
        e_x0 = max(_rel_rms(tx0[i, b], rx0[i, b]) for i in range(n_iter - 1))
        moved = _rel_rms(lat[b], plain[b].cpu())
        print(f"{case}, request {b} ({'dpm' if plus[b] else 'ddim eta 1'}, g {g[b]}, {n_iter} levels): first combined prediction {e_first:.3e}, end latent "
              f"{e_lat:.3e}, worst-step trace_x0 {e_x0:.3e}; distance from plain CFG {moved:.3e}")
        assert np.isfinite(e_first) and e_first <= FWD_TOL
        assert np.isfinite(e_lat) and e_lat <= TRAJ_TOL
        assert moved > e_lat, "the shaped trajectory is no farther from plain CFG than from its reference: the test shows nothing"


# ---- 6. the pipeline, the batcher, the accounting, the refusals ------------------------------------------------------------------------------------------
def test_pipeline_and_mixed_batcher_pictures_equal_the_one_prompt_call():
    from PIL import Image
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, DenoiserConfig, DiffusionTransformer, LTDConfig, RequestBatcher, VaeDecoderConfig
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(_dev())
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2).to(_dev())

    class Tok:
        def tokenize(self, prompts, truncate=True):                     # clip.tokenize stand-in: SOT, one id per character, EOT, zero padding
            t = torch.zeros(len(prompts), ccfg.context_length, dtype=torch.long)
            for i, p in enumerate(prompts):
                ids = [1 + (ord(ch) % 900) for ch in p][: ccfg.context_length - 2]
                t[i, 0] = ccfg.vocab_size - 2
                t[i, 1:1 + len(ids)] = torch.tensor(ids)
                t[i, 1 + len(ids)] = ccfg.vocab_size - 1
            return t

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(image_size=16, embed_dim=128, n_layers=2, n_channels=4)), vae=vae, clip_model=enc,
                                tokenizer=Tok(), run_device=_dev())
    prompts, seeds = ["a cute cat", "a red car", "a tall tree"], [3, 4, 5]
    arr = lambda p: np.asarray(p)
    shape = dict(guidance_rescale=0.7, apg_eta=0.0, apg_norm=2.5, apg_momentum=-0.5)
    pics = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5, **shape)
    assert len(pics) == 3 and all(isinstance(p, Image.Image) for p in pics)
    for i in range(3):
        alone = pipe.generate_image_from_text(prompts[i], class_guidance=6, seed=seeds[i], n_iter=5, **shape)
        assert np.array_equal(arr(pics[i]), arr(alone)), f"prompt {i}: the batched call's picture differs from the one-prompt call"
    plain = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5)
    assert all(not np.array_equal(arr(a), arr(b)) for a, b in zip(pics, plain)), "the shaped call gives the pictures of plain CFG"
    # per-prompt values: the neutral request keeps its plain picture
    per = dict(guidance_rescale=[0.7, 0.0, 0.7], apg_eta=[0.0, 1.0, 0.0], apg_norm=[2.5, 0.0, 2.5], apg_momentum=[-0.5, 0.0, -0.5])
    mixed = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5, **per)
    assert np.array_equal(arr(mixed[1]), arr(plain[1])) and np.array_equal(arr(mixed[0]), arr(pics[0])) and np.array_equal(arr(mixed[2]), arr(pics[2]))
    # the mixed batcher: one call, every ticket its solo picture
    rb = RequestBatcher(pipe, max_batch=8, mixed=True)
    t = [rb.submit(prompts[0], 6, seeds[0], 5, **shape), rb.submit(prompts[1], 6, seeds[1], 5), rb.submit(prompts[2], 4.5, seeds[2], 4, guidance_rescale=1.0)]
    assert len(rb.plan()) == 1
    got = rb.flush()
    assert np.array_equal(arr(got[t[0]]), arr(pics[0])) and np.array_equal(arr(got[t[1]]), arr(plain[1]))
    solo = pipe.generate_image_from_text(prompts[2], class_guidance=4.5, seed=seeds[2], n_iter=4, guidance_rescale=1.0)
    assert np.array_equal(arr(got[t[2]]), arr(solo))


def test_accounting_sample_rows_and_update_launches():
    """sample_rows are those of the entry it generalises; `update` launches = steps + the steps at which a running request is shaped and guided."""
    cfg, sd, m, gen = _model()
    eps, z0, labels = _inputs(4, seed=207)
    kw = dict(n_iter=[6, 4, 6, 3], class_guidance=[3.0, 4.5, 2.0, 6.0], seeds=eps, img_size=16)
    n = sum(kw["n_iter"])
    iv = [None, None, (0.3, 0.8), None]

    def launches(**more):
        gen.generate_latents_requests(labels, **kw, **more)                       # (allocations of a first call stay outside)
        m.set_profile(["update"])
        try:
            gen.generate_latents_requests(labels, **kw, **more)
            ms, k = m.get_profile("update")
        finally:
            m.set_profile([])
        return k, m.sample_rows()

    assert launches() == (6, (n, n))
    # every request shaped, no table: the CFG-doubled batch, a statistics launch at every step
    assert launches(guidance_rescale=0.7) == (12, (n, n))
    # only the 3-level request shaped: statistics at its 3 steps
    assert launches(guidance_rescale=[0, 0, 0, 0.7]) == (9, (n, n))
    # only request 2 shaped, guided inside (0.3, 0.8) only: statistics at the forwards whose level lies inside
    from transformer_latent_diffusion_amd import schedule
    inside = int((schedule.guidance_table(schedule.step_coefficients(schedule.noise_schedule(6, 1)), 2.0, (0.3, 0.8)) != 1.0).sum())
    assert 0 < inside < 6
    k, rows = launches(guidance_interval=iv, apg_eta=[1, 1, 0.0, 1], apg_momentum=[0, 0, -0.5, 0])
    gen.generate_latents_requests(labels, guidance_interval=iv, **kw)
    assert k == 6 + inside and rows == m.sample_rows() and rows == (n, n - (6 - inside)), (k, rows, inside)
    # neutral rows through the new entry: no statistics launch at all
    co = [schedule.step_coefficients(schedule.noise_schedule(c, 1)) for c in kw["n_iter"]]
    m.set_profile(["update"])
    try:
        m.sample_latents_requests(eps.to(_dev()), labels.to(_dev()), co, kw["class_guidance"], shape=[R.NEUTRAL] * 4)
        assert m.get_profile("update")[1] == 6
    finally:
        m.set_profile([])
    names = type(m).SAMPLER_PATH_NAMES
    bit = {v: k for k, v in names.items()}
    upd = sum(1 << i for i in names) | sum(1 << i for i, nm in enumerate(type(m).PATH_NAMES) if nm in ("update", "update_from", "update_from masked", "start_mix"))
    m.set_debug(True)
    try:
        gen.generate_latents_requests(labels, **kw, guidance_rescale=0.7)
        p_shaped = m.debug_paths()
    finally:
        m.set_debug(False)
    assert p_shaped & upd == 1 << bit["update_requests"], hex(p_shaped)
    print(f"update launches: plain 6, all shaped 12, one 3-level request 9, one request inside its interval {6 + inside}; sample rows {rows}")


def test_device_side_refusals_enqueue_nothing():
    from transformer_latent_diffusion_amd import _lib, schedule
    cfg, sd, m, gen = _model()
    eps, z0, labels = _inputs(4, seed=208)
    kw = dict(n_iter=[6, 4, 6, 3], class_guidance=3.0, seeds=eps, img_size=16, guidance_rescale=0.7, apg_momentum=-0.5)
    want = gen.generate_latents_requests(labels, **kw)
    L, h, cap, dev = _lib.lib(), m._engine, m._engine_batch, _dev()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Rq = _lib.TldSampleRequest
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())

    def call(B, recs, n_max, table, noise, lab, out, guidance=None, init=None, mask=None, shape=None):
        arr = (Rq * B)(*recs)
        s = np.tile(np.array([0.0, 2.5, -0.5, 0.7], np.float32), (B, 1)) if shape is None else shape
        rc = L.tld_sample_requests_shaped(h, vp(noise), vp(init), vp(mask), vp(lab), None, arr, fp(table), fp(guidance), None, None, fp(s), n_max, 0.0, 0.0,
                                          vp(out), B, None, None, stream)
        return rc, L.tld_last_error().decode()

    co4 = schedule.step_coefficients(schedule.noise_schedule(4, 1))
    Bbig = cap // 2 + 1
    big = torch.zeros(Bbig, 4, 16, 16, device=dev)
    sent_big = torch.full_like(big, 7.0)
    rc, msg = call(Bbig, [Rq(4, 3.0, 1.0, 0)] * Bbig, 4, np.tile(co4, (Bbig, 1, 1)), big, torch.zeros(Bbig, 768, device=dev), sent_big)
    assert rc == 1 and "max_batch" in msg, (rc, msg)
    Bg = cap - 1
    xg = torch.zeros(Bg, 4, 16, 16, device=dev)
    gt = np.ones((Bg, 4), dtype=np.float32)
    gt[:2, 1] = 3.0                                                                # step 1 runs Bg + 2 samples
    sent_g = torch.full_like(xg, 7.0)
    rc, msg = call(Bg, [Rq(4, 3.0, 1.0, 0)] * Bg, 4, np.tile(co4, (Bg, 1, 1)), xg, torch.zeros(Bg, 768, device=dev), sent_g, guidance=gt)
    assert rc == 1 and "step 1" in msg and "max_batch" in msg, (rc, msg)
    x4, lab4 = eps.to(dev).contiguous(), labels.to(dev).contiguous()
    sentinel = torch.full_like(x4, 7.0)
    tab4 = np.tile(co4, (4, 1, 1))
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, lab4, sentinel, mask=torch.ones(4, 1, 16, 16, device=dev))
    assert rc == 1 and "init_latent" in msg, (rc, msg)
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, lab4, None)
    assert rc == 1 and "null" in msg, (rc, msg)
    bad = np.tile(np.array([0.0, 2.5, -0.5, 0.7], np.float32), (4, 1))
    bad[2, 3] = 1.5
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, lab4, sentinel, shape=bad)
    assert rc == 1 and "request 2" in msg and "phi" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()) and bool((sent_big == 7.0).all()) and bool((sent_g == 7.0).all()), "a refused call wrote its output"
    assert torch.equal(gen.generate_latents_requests(labels, **kw), want)         # a following valid call is bitwise right: the momentum restarts at zero

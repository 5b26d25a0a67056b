"""GPU: noise injected inside the sampler's step (tld_sample_requests_stochastic) -- SDE DPM-Solver++(2M) and DDIM with eta.

The defining rules are bitwise.  All-zero noise coefficients are the guided / plain request entry and generate_latents.  One nonzero coefficient at
step k leaves every earlier state alone and makes x_t = fl32(x_t_det + fl32(e z)) there, z the normals tld_debug_sampler_noise returns for the same
(key, step) from the same device function, before the mask blend.  Request b of a mixed call equals the request alone with the same key.  The normals
themselves are held to the bound and the float64 statement of tests/test_gpu_batch_prep.py (same functions), and the trajectories at eta = 1 to the
contract tolerances of tests/test_gpu_requests.py against tests/stochastic_ref.py fed the device's z.  Every test prints the figures it asserts."""
import ctypes as C
from dataclasses import asdict

import numpy as np
import pytest
import torch

import stochastic_ref as S
from conftest import cfg_from_arr, load_golden, synth_weights

pytestmark = pytest.mark.gpu

TRAJ_TOL = 6e-2          # the contract tolerance of a multi-step CFG trajectory (tests/test_gpu_requests.py)
FWD_TOL = 2e-2           # ... of one forward
KS_ALPHA_001 = 1.95      # the alpha = 0.001 critical value of sqrt(n) D_n (tests/test_gpu_batch_prep.py)

TINY, BIG = "g2_tiny32_sampler.npz", "g5_100m.npz"
_CACHE = {}


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(fixture, low_latency=0):
    key = (fixture, low_latency)
    if key not in _CACHE:
        from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
        g = load_golden(fixture)
        cfg = cfg_from_arr(g["cfg"])
        sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
        m = Denoiser(**asdict(cfg)).to(_dev())
        if low_latency:
            m.set_low_latency(low_latency)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        _CACHE[key] = (cfg, sd, m, DiffusionGenerator(m, None, _dev(), torch.float32))
    return _CACHE[key]


def _inputs(B, S_=32, seed=101):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S_, S_, generator=gen)
    z0 = torch.randn(B, 4, S_, S_, generator=gen) * 0.5
    labels = torch.randn(B, 768, generator=gen) * 0.5
    return eps, z0, labels


def _rect_mask(S_=32):
    m = torch.zeros(1, S_, S_)
    m[:, 5:21, 3:17] = 1
    return m


def _device_noise(keys, steps, img):
    """tld_debug_sampler_noise: z [len(keys), img] fp32 on the host"""
    from transformer_latent_diffusion_amd import _lib
    dev = _dev()
    k = torch.tensor(np.array(keys, dtype=np.uint64).view(np.int64), device=dev)
    s = torch.tensor(np.array(steps, dtype=np.uint32).view(np.int32), device=dev)
    out = torch.empty(len(keys), img, device=dev)
    _lib.check(_lib.lib().tld_debug_sampler_noise(C.c_void_p(k.data_ptr()), C.c_void_p(s.data_ptr()), len(keys), img, C.c_void_p(out.data_ptr()),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_debug_sampler_noise")
    torch.cuda.synchronize()
    return out.cpu()


def _equal3(a, b, what):
    for u, v, name in zip(a, b, ("end latent", "trace_x0", "trace_xt")):
        assert u.shape == v.shape and torch.equal(u, v), f"{what}: {name} differs"


# ---- 1. all-zero coefficients are today's entries ---------------------------------------------------------------------------------------------------------
def test_all_zero_coefficients_are_the_guided_the_plain_and_the_uniform_entry():
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    B = 4
    eps, z0, labels = (t.to(_dev()) for t in _inputs(B))
    n_iter, guid, plus = [6, 4, 6, 3], [3.0, 4.5, 1.0, 6.0], [True, True, False, True]
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1), p) for n, p in zip(n_iter, plus)]
    zeros, keys = [np.zeros(n, np.float32) for n in n_iter], [11, 12, 13, 14]
    common = dict(sharp_f=0.1, bright_f=0.1, trace=True)
    # (a) the guided entry on tables with skipped steps
    tables = [np.array([3.0, 3.0, 1.0, 1.0, 3.0, 1.0], np.float32), np.array([1.0, 4.5, 4.5, 1.0], np.float32), np.ones(6, np.float32),
              np.array([6.0, 1.0, 6.0], np.float32)]
    want = m.sample_latents_requests(eps, labels, coeffs, None, guidance_steps=tables, **common)
    rows_want = m.sample_rows()
    got = m.sample_latents_requests(eps, labels, coeffs, None, guidance_steps=tables, noise_coeffs=zeros, noise_keys=keys, **common)
    rows_got = m.sample_rows()
    _equal3(got, want, "all-zero coefficients beside tld_sample_requests_guided")
    assert rows_got == rows_want and rows_got[1] < rows_got[0], (rows_got, rows_want)
    # (b) guidance NULL: tld_sample_requests, the 2 B_i batch with no skipping (request 2 is guided at 1.0 and still runs its pair)
    want = m.sample_latents_requests(eps, labels, coeffs, guid, **common)
    rows_want = m.sample_rows()
    got = m.sample_latents_requests(eps, labels, coeffs, guid, noise_coeffs=zeros, noise_keys=keys, **common)
    rows_got = m.sample_rows()
    _equal3(got, want, "all-zero coefficients, guidance NULL, beside tld_sample_requests")
    assert rows_got == rows_want == (sum(n_iter), sum(n_iter)), (rows_got, rows_want)
    # (c) generate_latents: a uniform batch
    kw = dict(n_iter=6, class_guidance=3.0, img_size=32, sharp_f=0.1, bright_f=0.1, seeds=eps, trace=True)
    want = gen.generate_latents(labels, num_imgs=B, **kw)
    co = schedule.step_coefficients(schedule.noise_schedule(6, 1))
    got = m.sample_latents_requests(eps, labels, [co] * B, [3.0] * B, noise_coeffs=[np.zeros(6, np.float32)] * B, noise_keys=keys, **common)
    _equal3(got, want, "all-zero coefficients beside generate_latents")
    print(f"all-zero coefficients: bitwise equal to the guided entry (sample rows {rows_want}), the plain entry and generate_latents")


# ---- 2. the normals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def normals():
    keys = [0x1234 + 7 * b if b < 8 else (0xFEDCBA9876543210 ^ b) for b in range(16)]
    steps = [b % 4 for b in range(16)]
    assert len(set(zip(keys, steps))) == 16
    return keys, steps, _device_noise(keys, steps, 1 << 16)


def test_normals_against_float64_box_muller_on_the_same_philox_bits(normals):
    """|z - float64 Box-Muller from the unrounded uniforms| <= 1e-5: the bound and the float64 statement of tests/test_gpu_batch_prep.py, for the
    same functions (its error budget, about 4e-6 at radius <= 5.9, is written there)."""
    keys, steps, z = normals
    z = z.numpy().astype(np.float64)
    assert z.size == 1 << 20
    err = max(np.abs(z[b] - S.noise_f64(keys[b], steps[b], z.shape[1])).max() for b in range(16))
    print(f"sampler noise: max |fp32 - float64| {err:.3e} over 2^20 values; max |z| {np.abs(z).max():.3f}")
    assert err <= 1e-5
    assert np.abs(z).max() <= 5.9


def test_normals_pass_kolmogorov_smirnov(normals):
    from scipy import stats
    z = np.sort(normals[2].numpy().reshape(-1).astype(np.float64))
    n = z.size
    f = stats.norm.cdf(z)
    d = max(float((np.arange(1, n + 1) / n - f).max()), float((f - np.arange(n) / n).max()))
    print(f"sampler noise: n {n}, KS {d:.3e} against {KS_ALPHA_001 / np.sqrt(n):.3e}; mean {z.mean():.2e}, var {z.var():.5f}")
    assert d <= KS_ALPHA_001 / np.sqrt(n)


def test_streams_are_distinct_repeatable_and_independent_of_the_batch(normals):
    keys, steps, z = normals
    flat = z.numpy()
    for a in range(16):
        for b in range(a + 1, 16):
            same = float((flat[a] == flat[b]).mean())
            assert same < 1e-3, f"streams {a} and {b} share {same:.4f} of their values"
    # the same key at another step, and another key at the same step
    other = _device_noise([keys[0], keys[0] ^ (1 << 40)], [steps[0] + 1, steps[0]], 4096)
    assert float((other[0] == z[0, :4096]).float().mean()) < 1e-2 and float((other[1] == z[0, :4096]).float().mean()) < 1e-2
    again = _device_noise(keys, steps, 1 << 16)
    assert torch.equal(again, z), "two identical calls differ"
    sub = _device_noise([keys[9], keys[2]], [steps[9], steps[2]], 1 << 16)
    assert torch.equal(sub[0], z[9]) and torch.equal(sub[1], z[2]), "a stream depends on its place in the batch or on the batch size"
    # an image that is no multiple of 4 elements: a prefix of the same stream, the last quad cut
    odd = _device_noise([keys[3]], [steps[3]], 4099)
    assert torch.equal(odd[0], z[3, :4099])


# ---- 3. the step, bitwise -------------------------------------------------------------------------------------------------------------------------------
def _direct(m, eps, labels, coeffs, guid, ecoef, keys, out, tx0, txt, z0=None, mask=None):
    """tld_sample_requests_stochastic straight through ctypes on the caller's device tensors (records already in engine order, guidance NULL)"""
    from transformer_latent_diffusion_amd import _lib
    B, n_max = eps.shape[0], coeffs[0].shape[0]
    table, etab = np.zeros((B, n_max, 6), dtype=np.float32), np.zeros((B, n_max), dtype=np.float32)
    recs = (_lib.TldSampleRequest * B)()
    for b in range(B):
        table[b, :coeffs[b].shape[0]] = coeffs[b]
        etab[b, :len(ecoef[b])] = ecoef[b]
        recs[b] = _lib.TldSampleRequest(coeffs[b].shape[0], guid[b], 1.0, 0)
    karr = np.array(keys, dtype=np.uint64)
    h = m._ensure_engine(2 * B, _dev())
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    rc = _lib.lib().tld_sample_requests_stochastic(h, vp(eps), vp(z0), vp(mask), vp(labels), None, recs, fp(table), None, fp(etab),
                                                   karr.ctypes.data_as(C.POINTER(C.c_uint64)), n_max, 0.1, 0.1, vp(out), B, vp(tx0), vp(txt),
                                                   C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream))
    assert rc == 0, _lib.lib().tld_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_one_noisy_step_is_the_deterministic_state_plus_e_z(masked):
    """Deterministic coefficients, noise_coeff nonzero at exactly one step k (0, a middle one, the last inner step), beside the all-zero call: the
    states before k are equal, and at k x_t = fl32(x_t_det + fl32(e z)) -- numpy float32, one multiply and one add -- with z from
    tld_debug_sampler_noise.  With a mask the sum is taken before the blend: where m = 0 the state is the deterministic call's, where m = 1 the
    formula holds.  Run on the 16-byte instantiation and, through trace_xt and out_latent views that start 4 bytes into their buffers, on the
    scalar one (as test_scalar_instantiation_through_an_odd_offset_view reaches it)."""
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    dev = _dev()
    eps, z0, labels = _inputs(2, seed=103)
    eps, z0, labels = eps.to(dev).contiguous(), z0.to(dev).contiguous(), labels.to(dev).contiguous()
    mask = torch.stack([_rect_mask(), 1 - _rect_mask()]).to(dev).contiguous() if masked else None
    counts = (6, 4)
    coeffs = [schedule.step_coefficients(schedule.noise_schedule(n, 1)) for n in counts]
    guid, keys, e_val = [3.0, 4.5], [0xABCDEF0123456789, 77], np.float32(0.37)
    n = eps.numel()
    img = n // 2

    def run(ecoef, odd):
        out, tx0 = torch.empty_like(eps), torch.zeros((5,) + tuple(eps.shape), device=dev)
        if not odd:
            txt = torch.zeros_like(tx0)
            _direct(m, eps, labels, coeffs, guid, ecoef, keys, out, tx0, txt, z0 if masked else None, mask)
            return out, tx0, txt
        buf_o, buf_t = torch.zeros(n + 4, device=dev), torch.zeros(5 * n + 4, device=dev)
        out_u, txt_u = buf_o[1:1 + n].view_as(eps), buf_t[1:1 + 5 * n].view(5, *eps.shape)
        assert out_u.data_ptr() % 16 == 4 and txt_u.data_ptr() % 16 == 4
        _direct(m, eps, labels, coeffs, guid, ecoef, keys, out_u, tx0, txt_u, z0 if masked else None, mask)
        assert float(buf_o[0]) == 0.0 and float(buf_o[-3:].abs().max()) == 0.0 and float(buf_t[0]) == 0.0 and float(buf_t[-3:].abs().max()) == 0.0
        return out_u.clone(), tx0, txt_u.clone()

    det = run([np.zeros(c, np.float32) for c in counts], False)
    for k in (0, 2, 4):
        who = [b for b in range(2) if k < counts[b] - 1]              # k = 4 is request 0's last inner step; request 1 has finished
        ecoef = [np.zeros(c, np.float32) for c in counts]
        for b in who:
            ecoef[b][k] = e_val
        zk = _device_noise([keys[b] for b in who], [k] * len(who), img).numpy().reshape(len(who), 4, 32, 32)
        for odd in (False, True):
            out, tx0, txt = run(ecoef, odd)
            assert torch.equal(txt[:k], det[2][:k]) and torch.equal(tx0[:k + 1], det[1][:k + 1]), f"k = {k}: a state before the noisy step moved"
            for j, b in enumerate(who):
                xt_det, xt = det[2][k, b].cpu().numpy(), txt[k, b].cpu().numpy()
                want = (xt_det + (e_val * zk[j]).astype(np.float32)).astype(np.float32)
                if masked:
                    one = (mask[b].cpu().numpy() == 1.0).repeat(4, axis=0)
                    assert np.array_equal(xt[~one], xt_det[~one]), f"k = {k}, request {b}: the kept region moved"
                    assert np.array_equal(xt[one], want[one]), f"k = {k}, request {b}: the regenerated region is not x_t + e z"
                    assert one.any() and (~one).any()
                else:
                    assert np.array_equal(xt, want), f"k = {k}, request {b}: x_t is not fl32(x_t_det + fl32(e z))"
                assert not np.array_equal(xt, xt_det)
            for b in set(range(2)) - set(who):
                assert torch.equal(txt[:, b], det[2][:, b]) and torch.equal(out[b], det[0][b])
            if k < 3:
                assert not torch.equal(out[1], det[0][1])
            assert not torch.equal(out[0], det[0][0])
            if not odd:
                vec = (out, tx0, txt)
            else:
                _equal3((out, tx0, txt), vec, f"k = {k}: the scalar instantiation beside the 16-byte one")
    print(f"one noisy step ({'masked' if masked else 'plain'}): k = 0, 2, 4 at V = 4 and V = 1: x_t == fl32(x_t_det + fl32(e z)) bit for bit")


# ---- 4. a request of a mixed call is the request alone -----------------------------------------------------------------------------------------------
MIX = dict(n_iter=[8, 5, 8, 3, 5], class_guidance=[3.0, 4.5, 6.0, 3.0, 1.5], use_ddpm_plus=[True, True, False, True, True], exponent=[1, 1, 1, 1, 2],
           eta=[1.0, 0.0, 0.5, 2.0, 1.0], strength=[None, 0.65, None, None, None], guidance_interval=[None, None, (0.3, 0.8), None, (0.0, 0.5)])
MIX_KEYS = [5, 6 | (3 << 32), 7, 8, (1 << 64) - 1]


def _mix_operands(labels, z0):
    neg = [None, None, labels[0] * 0.5, None, None]
    mask = [None, None, None, _rect_mask(), None]
    init = [None, z0[1], None, z0[3], None]
    return neg, mask, init


def _call_mixed(gen, eps, labels, z0, idx, kw=MIX, keys=MIX_KEYS):
    neg, mask, init = _mix_operands(labels, z0)
    pick = lambda v: [v[i] for i in idx]
    return gen.generate_latents_requests(labels[idx], seeds=eps[idx], img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, negative_labels=pick(neg),
                                         mask=pick(mask), init_latents=pick(init), noise_seeds=pick(keys), **{k: pick(v) for k, v in kw.items()})


def test_request_of_a_mixed_call_equals_the_request_alone_and_order_does_not_matter():
    """Different n_iter, eta including 0, guidance intervals, one image-to-image, one masked, one negative label, one DDIM request."""
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(5, seed=104)
    lat, tx0, txt = _call_mixed(gen, eps, labels, z0, list(range(5)))
    assert torch.isfinite(lat).all()
    for b in range(5):
        a, ax0, axt = _call_mixed(gen, eps, labels, z0, [b])
        nb = ax0.shape[0]
        assert torch.equal(lat[b], a[0]) and torch.equal(tx0[:nb, b], ax0[:, 0]) and torch.equal(txt[:nb, b], axt[:, 0]), f"request {b} differs from the request alone"
        assert not tx0[nb:, b].any() and not txt[nb:, b].any()
    perm = [3, 0, 4, 2, 1]
    second = _call_mixed(gen, eps, labels, z0, perm)
    for u, v in zip((lat, tx0, txt), second):
        idx = (slice(None), perm) if u.dim() == 5 else (perm,)
        assert torch.equal(u[idx], v), "a request's result depends on the order of submission"
    # the noise is there: the same call at eta = 0 differs in the requests that had eta > 0, and only there; another key moves only its request
    det = _call_mixed(gen, eps, labels, z0, list(range(5)), kw=dict(MIX, eta=[0.0] * 5))
    moved = [not torch.equal(lat[b], det[0][b]) for b in range(5)]
    assert moved == [e > 0 for e in MIX["eta"]], moved
    rekey = _call_mixed(gen, eps, labels, z0, list(range(5)), keys=MIX_KEYS[:2] + [99] + MIX_KEYS[3:])
    assert [not torch.equal(lat[b], rekey[0][b]) for b in range(5)] == [False, False, True, False, False]
    print("mixed call: 5 requests (eta 1, 0, 0.5, 2, 1) bitwise equal to each request alone, in either order")


def test_mixed_call_in_low_latency_class_1():
    cfg, sd, m, gen = _model(BIG, low_latency=1)
    eps, z0, labels = _inputs(3, seed=105)
    kw = dict(n_iter=[4, 3, 4], class_guidance=[6.0, 3.0, 4.5], use_ddpm_plus=[True, True, False], eta=[1.0, 0.0, 0.5], img_size=32, sharp_f=0.1,
              bright_f=0.1, trace=True)
    keys = [21, 22, 23]
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, noise_seeds=keys, **kw)
    for b in range(3):
        solo = gen.generate_latents_requests(labels[b:b + 1], seeds=eps[b:b + 1], noise_seeds=keys[b:b + 1],
                                             **{k: ([v[b]] if isinstance(v, list) else v) for k, v in kw.items()})
        nb = solo[1].shape[0]
        assert torch.equal(lat[b], solo[0][0]) and torch.equal(txt[:nb, b], solo[2][:, 0]), f"low-latency class 1: request {b} differs from the request alone"


# ---- 5. against the CPU reference loop fed the device's z -------------------------------------------------------------------------------------------
def _rel_rms(a, b):
    a, b = a.double(), b.double()
    return float((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30))


def test_trajectory_at_eta_one_vs_reference_loop():
    """eta = 1, DPM-Solver++(2M) SDE and first-order (DDIM eta = 1), 6 levels, guidance 3.0 / 4.5, tiny weights, against tests/stochastic_ref.py
    fed the z of tld_debug_sampler_noise: the contract tolerances of tests/test_gpu_requests.py, no regression bound (the figures are printed)."""
    from oracle.torch_ref import TorchRefDenoiser
    from transformer_latent_diffusion_amd import schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(2, seed=106)
    g, plus, keys, n_iter = [3.0, 4.5], [True, False], [31, 32 | (1 << 32)], 6
    lat, tx0, txt = gen.generate_latents_requests(labels, seeds=eps, n_iter=n_iter, class_guidance=g, use_ddpm_plus=plus, eta=1.0, noise_seeds=keys,
                                                  img_size=32, sharp_f=0.1, bright_f=0.1, trace=True)
    ref = TorchRefDenoiser(asdict(cfg), sd)
    levels = [schedule.noise_schedule(n_iter, 1)] * 2
    z = [[zz.reshape(4, 32, 32) for zz in _device_noise([keys[b]] * (n_iter - 1), list(range(n_iter - 1)), 4 * 32 * 32)] for b in range(2)]
    rlat, rx0, rxt = S.sample_requests(ref, eps, None, None, labels, None, levels, [1.0, 1.0], [[g[b]] * n_iter for b in range(2)], plus, [1.0, 1.0], z,
                                       0.1, 0.1, trace=True)
    lat, tx0, txt = lat.cpu(), tx0.cpu(), txt.cpu()
    for b in range(2):
        e_first = _rel_rms(tx0[0, b], rx0[0, b])
        e_lat = _rel_rms(lat[b], rlat[b])
        e_x0 = max(_rel_rms(tx0[i, b], rx0[i, b]) for i in range(n_iter - 1))
        e_xt = max(_rel_rms(txt[i, b], rxt[i, b]) for i in range(n_iter - 1))
        print(f"eta = 1 trajectory, request {b} ({'dpm' if plus[b] else 'ddim'}, g {g[b]}, {n_iter} levels): first combined prediction {e_first:.3e}, "
              f"end latent {e_lat:.3e}, worst-step trace_x0 {e_x0:.3e}, trace_xt {e_xt:.3e}")
        assert np.isfinite(e_first) and e_first <= FWD_TOL
        assert np.isfinite(e_lat) and e_lat <= TRAJ_TOL


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------------------------
def test_pipeline_eta_pictures_equal_the_one_prompt_call():
    from PIL import Image
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, DenoiserConfig, DiffusionTransformer, LTDConfig, VaeDecoderConfig
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

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=vae, clip_model=enc, tokenizer=Tok(), run_device=_dev())
    prompts, seeds = ["a cute cat", "a red car", "a tall tree"], [3, 4, 5]
    arr = lambda p: np.asarray(p)
    pics = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5, eta=1)
    assert len(pics) == 3 and all(isinstance(p, Image.Image) for p in pics)
    for i in range(3):
        alone = pipe.generate_image_from_text(prompts[i], class_guidance=6, seed=seeds[i], n_iter=5, eta=1)
        assert np.array_equal(arr(pics[i]), arr(alone)), f"prompt {i}: the batched call's picture differs from the one-prompt call at eta = 1"
    det = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5)
    assert all(not np.array_equal(arr(a), arr(b)) for a, b in zip(pics, det)), "eta = 1 gives the pictures of eta = 0"
    again = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5, eta=1)
    assert all(np.array_equal(arr(a), arr(b)) for a, b in zip(pics, again)), "two identical calls differ"
    other = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=[13, 14, 15], n_iter=5, eta=1)
    assert all(not np.array_equal(arr(a), arr(b)) for a, b in zip(pics, other))
    # per-prompt eta: the eta = 0 request keeps its deterministic picture
    mixed = pipe.generate_images_from_texts(prompts, class_guidance=6, seeds=seeds, n_iter=5, eta=[1, 0, 1])
    assert np.array_equal(arr(mixed[1]), arr(det[1])) and np.array_equal(arr(mixed[0]), arr(pics[0])) and np.array_equal(arr(mixed[2]), arr(pics[2]))


# ---- 7. accounting ----------------------------------------------------------------------------------------------------------------------------------------
def test_sample_rows_launches_and_path_bits_are_those_of_the_entry_it_generalises():
    from transformer_latent_diffusion_amd import Denoiser, schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(4, seed=107)
    kw = dict(n_iter=[6, 4, 6, 3], class_guidance=[3.0, 4.5, 2.0, 6.0], seeds=eps, img_size=32)
    sde = dict(eta=[1.0, 0.5, 0.0, 2.0], noise_seeds=[1, 2, 3, 4])
    n = sum(kw["n_iter"])
    gen.generate_latents_requests(labels, **kw, **sde)
    assert m.sample_rows() == (n, n)                                              # guidance NULL: the CFG-doubled batch of tld_sample_requests
    iv = [(0.3, 0.8), None, (0.0, 0.5), None]
    gen.generate_latents_requests(labels, guidance_interval=iv, **kw)
    rows_guided = m.sample_rows()
    gen.generate_latents_requests(labels, guidance_interval=iv, **kw, **sde)
    assert m.sample_rows() == rows_guided and rows_guided[0] == n and rows_guided[1] < n
    m.set_profile(["update"])
    try:
        gen.generate_latents_requests(labels, **kw, **sde)
        ms, launches = m.get_profile("update")
    finally:
        m.set_profile([])
    assert launches == max(kw["n_iter"]) and ms > 0.0, (launches, ms)             # still one launch per step
    names = Denoiser.SAMPLER_PATH_NAMES
    bit = {v: k for k, v in names.items()}
    upd = sum(1 << i for i in names) | sum(1 << i for i, nm in enumerate(Denoiser.PATH_NAMES) if nm in ("update", "update_from", "update_from masked", "start_mix"))
    m.set_debug(True)
    try:
        gen.generate_latents_requests(labels, **kw)
        p_plain = m.debug_paths()
        gen.generate_latents_requests(labels, **kw, **sde)
        p_sde = m.debug_paths()
        gen.generate_latents_requests(labels, init_latents=z0, strength=[None, 0.65, None, None], mask=[None, _rect_mask(), None, None], **kw, **sde)
        p_mask = m.debug_paths()
    finally:
        m.set_debug(False)
    print(f"sample rows: stochastic ({n}, {n}), with intervals {rows_guided}; update launches {launches}; launch paths plain {p_plain:#x}, stochastic {p_sde:#x}, "
          f"stochastic masked {p_mask:#x}")
    assert p_sde & upd == p_plain & upd == 1 << bit["update_requests"]
    assert p_mask & upd == (1 << bit["update_requests masked"]) | (1 << bit["start_mix per request"])


# ---- 8. refusals on the device side -------------------------------------------------------------------------------------------------------------------------
def test_device_side_refusals_enqueue_nothing():
    from transformer_latent_diffusion_amd import _lib, schedule
    cfg, sd, m, gen = _model(TINY)
    eps, z0, labels = _inputs(4, seed=108)
    kw = dict(n_iter=[6, 4, 6, 3], class_guidance=3.0, seeds=eps, img_size=32, eta=1.0, noise_seeds=[1, 2, 3, 4])
    want = gen.generate_latents_requests(labels, **kw)
    L, h, cap, dev = _lib.lib(), m._engine, m._engine_batch, _dev()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    Rq = _lib.TldSampleRequest
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    vp = lambda t: C.c_void_p(None if t is None else t.data_ptr())

    def call(B, recs, n_max, table, noise, lab, out, guidance=None, init=None, mask=None):
        arr = (Rq * B)(*recs)
        e = np.zeros((B, n_max), dtype=np.float32)
        for b, r in enumerate(recs):
            e[b, :r.n_levels - 1] = 0.2
        keys = np.arange(B, dtype=np.uint64)
        rc = L.tld_sample_requests_stochastic(h, vp(noise), vp(init), vp(mask), vp(lab), None, arr, fp(table), fp(guidance), fp(e),
                                              keys.ctypes.data_as(C.POINTER(C.c_uint64)), n_max, 0.0, 0.0, vp(out), B, None, None, stream)
        return rc, L.tld_last_error().decode()

    co4 = schedule.step_coefficients(schedule.noise_schedule(4, 1), True, eta=1.0)[0]
    # guidance NULL: 2 B > max_batch, the rule of tld_sample_requests
    Bbig = cap // 2 + 1
    big = torch.zeros(Bbig, 4, 32, 32, device=dev)
    sent_big = torch.full_like(big, 7.0)
    rc, msg = call(Bbig, [Rq(4, 3.0, 1.0, 0)] * Bbig, 4, np.tile(co4, (Bbig, 1, 1)), big, torch.zeros(Bbig, 768, device=dev), sent_big)
    assert rc == 1 and "max_batch" in msg, (rc, msg)
    # with a table: the largest step of the guided call decides
    Bg = cap - 1
    xg = torch.zeros(Bg, 4, 32, 32, device=dev)
    gt = np.ones((Bg, 4), dtype=np.float32)
    gt[:2, 1] = 3.0                                                                # step 1 runs Bg + 2 samples
    sent_g = torch.full_like(xg, 7.0)
    rc, msg = call(Bg, [Rq(4, 3.0, 1.0, 0)] * Bg, 4, np.tile(co4, (Bg, 1, 1)), xg, torch.zeros(Bg, 768, device=dev), sent_g, guidance=gt)
    assert rc == 1 and "step 1" in msg and "max_batch" in msg, (rc, msg)
    # more than 1024 conditioning rows
    n = 300
    tab = np.zeros((4, n, 6), dtype=np.float32)
    for b in range(4):
        tab[b] = schedule.step_coefficients([0.99 - 1e-4 * (4 * i + b) for i in range(n)])
    x4 = eps.to(dev).contiguous()
    sentinel = torch.full_like(x4, 7.0)
    lab4 = labels.to(dev).contiguous()
    rc, msg = call(4, [Rq(n, 3.0, 1.0, 0)] * 4, n, tab, x4, lab4, sentinel)
    assert rc == 1 and "1205" in msg and "1024" in msg, (rc, msg)
    # a mask without init_latent, and a NULL output
    tab4 = np.tile(co4, (4, 1, 1))
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, lab4, sentinel, mask=torch.ones(4, 1, 32, 32, device=dev))
    assert rc == 1 and "init_latent" in msg, (rc, msg)
    rc, msg = call(4, [Rq(4, 3.0, 1.0, 0)] * 4, 4, tab4, x4, lab4, None)
    assert rc == 1 and "null" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all()) and bool((sent_big == 7.0).all()) and bool((sent_g == 7.0).all()), "a refused call wrote its output"
    assert torch.equal(gen.generate_latents_requests(labels, **kw), want)         # a following valid call is bitwise right

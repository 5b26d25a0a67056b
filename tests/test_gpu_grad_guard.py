"""GPU: the guarded optimizer step -- tld_train_grad_guard (global gradient norm in double, clip_grad_norm_ coefficient, non-finite skip,
Adam's step count on the device) and tld_train_adam_ema_guarded -- on raw vectors through the C ABI and through ``Trainer``.

Reference: tests/grad_guard_ref.py (float64 numpy; held against torch's clip_grad_norm_ + Adam by tests/test_grad_guard_host.py).
Bounds: the norm to 1e-12 relative (at 2^24 + 5 elements a thread adds fewer than 70 doubles serially and the trees add at most 26
levels: fewer than 100 roundings of 1.1e-16; an fp32 accumulator misses it by five orders of magnitude); the clipped first moment to 2^-22
relative (three fp32 roundings); parameters and EMA to 5e-7 absolute, the bound tests/test_gpu_train.py holds the same arithmetic to."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from test_gpu_parity import _dev
from test_gpu_train import _g15, _trainer
from transformer_latent_diffusion_amd import _lib

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, ALPHA = (R.f32(x) for x in (3e-4, 0.9, 0.999, 1e-8, 0.999))       # what the float arguments carry
UPDATE_TOL = 5e-7


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _state():
    return torch.zeros(_lib.TRAIN_OPT_STATE_DOUBLES, dtype=torch.float64, device=_dev())


def _guard(g, st, scale=1.0, max_norm=0.0, skip=0):
    _lib.check(_lib.lib().tld_train_grad_guard(None, _p(g), g.numel(), scale, max_norm, skip, B1, B2, _p(st), _stream()), "tld_train_grad_guard")


def _adam(p, g, m, v, ema, st, scale=1.0):
    _lib.check(_lib.lib().tld_train_adam_ema_guarded(None, _p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), LR, B1, B2, EPS, ALPHA, scale, _p(st),
                                                     _stream()), "tld_train_adam_ema_guarded")


def _head(st):
    return st[:8].cpu().numpy()


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _wide(n, rng):
    """Magnitudes from 1e-30 to 3e38, both signs: the fp32 squares of either end underflow / overflow."""
    mag = 10.0 ** rng.uniform(-30.0, np.log10(3e38), n)
    mag[rng.integers(n)] = 3e38
    if n > 1:
        mag[(np.argmax(mag) + 1) % n] = 1e-30
    return (mag * rng.choice([-1.0, 1.0], n)).astype(np.float32)


# ---- raw vectors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1024, 4096, 4097, 4100, 2 ** 20 + 1, 2 ** 24 + 5])
def test_norm_in_double_is_exact_to_1e12_and_bitwise_repeatable(n):
    rng = np.random.default_rng(n)
    inputs = {"normal": (rng.standard_normal(n) * 1e-2).astype(np.float32), "wide": _wide(n, rng)}
    for kind, host in inputs.items():
        g = torch.from_numpy(host).to(_dev())
        for scale in (1.0, 1.0 / 3.0):
            ref = float(R.grad_norm(host, scale))
            st, st2 = _state(), _state()
            _guard(g, st, scale)
            _guard(g, st2, scale)
            h = _head(st)
            err = abs(h[R.NORM] - ref) / ref
            print(f"n={n} {kind} scale={scale:.3f}: norm {h[R.NORM]:.17g} ref {ref:.17g} rel err {err:.2e}")
            assert np.isfinite(ref) and ref > 0
            assert err <= 1e-12, (kind, scale, h[R.NORM], ref)
            assert torch.equal(_bits(st), _bits(st2))                       # partials and head, bit for bit
            assert h[R.T] == 1 and h[R.LAST_SKIPPED] == 0 and h[R.COEF] == 1.0 and h[R.SKIPPED] == 0 and h[7] == 0
            assert h[R.BC1] == 1.0 - B1 and abs(h[R.BC2] - (1.0 - B2)) <= 1e-15


N_BAD = 2 ** 20 + 1
CHUNK = ((N_BAD + R.PARTS - 1) // R.PARTS + 3) // 4 * 4                     # 1028: workgroup b sums [b * CHUNK, (b + 1) * CHUNK)
BAD_AT = {"first": 0, "last": N_BAD - 1, "chunk_first": 500 * CHUNK, "chunk_last": 501 * CHUNK - 1}


@pytest.fixture(scope="module")
def stepped():
    """Vectors and state after ONE good guarded step (t = 1, non-zero moments and bias corrections); never modified by the tests."""
    gen = torch.Generator().manual_seed(11)
    p = (torch.randn(N_BAD, generator=gen) * 0.05).to(_dev())
    g = (torch.randn(N_BAD, generator=gen) * 1e-2).to(_dev())
    m, v, ema, st = torch.zeros_like(p), torch.zeros_like(p), p.clone(), _state()
    _guard(g, st, 1.0, 1.0, 1)
    _adam(p, g, m, v, ema, st)
    assert _head(st)[R.T] == 1 and float(m.abs().max()) > 0
    return p, g, m, v, ema, st


@pytest.mark.parametrize("where", list(BAD_AT))
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_one_nonfinite_element_skips_the_step_and_touches_nothing(stepped, bad, where):
    p, g, m, v, ema, st = (t.clone() for t in stepped)
    before = [t.clone() for t in (p, m, v, ema)]
    h0 = st[:8].clone()
    g[BAD_AT[where]] = bad
    _guard(g, st, 1.0, 1.0, 1)
    _adam(p, g, m, v, ema, st)
    h = _head(st)
    assert h[R.LAST_SKIPPED] == 1 and h[R.SKIPPED] == h0[R.SKIPPED].item() + 1 and h[R.COEF] == 0 and not np.isfinite(h[R.NORM])
    for k in (R.T, R.BC1, R.BC2):
        assert torch.equal(_bits(st[k:k + 1]), _bits(h0[k:k + 1])), k
    for a, b in zip((p, m, v, ema), before):
        assert torch.equal(_bits(a), _bits(b))
    # and the next good step is applied: the flag is per step
    g[BAD_AT[where]] = 0.0
    _guard(g, st, 1.0, 1.0, 1)
    _adam(p, g, m, v, ema, st)
    h = _head(st)
    assert h[R.LAST_SKIPPED] == 0 and h[R.T] == 2 and h[R.SKIPPED] == 1 and not torch.equal(p, before[0])


def test_nan_with_the_skip_off_gives_a_nan_coefficient_as_torch_does(stepped):
    _, g, _, _, _, st = (t.clone() for t in stepped)
    g[12345] = float("nan")
    _guard(g, st, 1.0, 1.0, 0)
    h = _head(st)
    assert np.isnan(h[R.NORM]) and np.isnan(h[R.COEF]) and h[R.LAST_SKIPPED] == 0 and h[R.T] == 2 and h[R.SKIPPED] == 0


@pytest.mark.parametrize("ratio", [2.0, 0.5])
def test_first_moment_carries_the_clipped_gradient(ratio):
    """From zero moments exp_avg = (1 - beta1) * g * scale * coef: three fp32 roundings, 2^-22 relative per element."""
    n, scale = 4099, 1.0 / 3.0
    host = (np.random.default_rng(5).standard_normal(n) * 1e-2).astype(np.float32)
    norm = float(R.grad_norm(host, scale))
    max_norm = norm / ratio
    coef = min(1.0, max_norm / (norm + 1e-6))
    g = torch.from_numpy(host).to(_dev())
    p = torch.zeros(n, device=_dev()); m, v, st = torch.zeros_like(p), torch.zeros_like(p), _state()
    _guard(g, st, scale, max_norm, 1)
    _adam(p, g, m, v, None, st, scale)
    h = _head(st)
    if ratio < 1:
        assert h[R.COEF] == 1.0
    else:
        assert abs(h[R.COEF] - coef) <= 1e-12 * coef and 0.49 < coef < 0.5
    want = host.astype(np.float64) * R.f32(scale) * coef
    got = m.cpu().numpy().astype(np.float64) / float(np.float32(1.0) - np.float32(B1))
    rel = np.abs(got - want) / np.abs(want)
    print(f"norm / max_norm = {ratio}: coef {h[R.COEF]:.17g}, worst first-moment error {rel.max():.3e} (bound {2.0 ** -22:.3e})")
    assert rel.max() <= 2.0 ** -22


def _padded(host, off=4, pad=8):
    """A device vector inside a larger buffer of sentinels (off floats in front: 4 keeps 16-byte alignment, 1 breaks it)."""
    full = torch.full((off + host.size + pad,), 7.5, dtype=torch.float32, device=_dev())
    full[off:off + host.size] = torch.from_numpy(host.astype(np.float32)).to(_dev())
    return full, full[off:off + host.size]


def _sentinels_intact(full, n, off):
    return bool((full[:off] == 7.5).all()) and bool((full[off + n:] == 7.5).all())


@pytest.mark.parametrize("n,off", [(2 ** 20, 4), (2 ** 20 + 1, 4), (2 ** 20 + 3, 4), (1001, 1)])
def test_two_clipped_steps_vs_float64_reference_and_the_idle_guard_vs_the_plain_kernel(n, off):
    """n = 4k, 4k + 1, 4k + 3: the 16-byte path and its tail; off = 1: vectors that are only 4-byte aligned take the scalar kernel."""
    rng = np.random.default_rng(n)
    p0 = rng.standard_normal(n) * 0.05
    grads = [(rng.standard_normal(n) * 1e-2).astype(np.float32) for _ in range(2)]
    max_norm = 0.5 * float(R.grad_norm(grads[0]))
    (pf, p), (mf, m), (vf, v), (ef, ema) = (_padded(a, off) for a in (p0, np.zeros(n), np.zeros(n), p0))
    plain = [t.clone() for t in (p, m, v, ema)]                            # aligned copies for tld_train_adam_ema
    idle = [t.clone() for t in plain]
    st, st_idle = _state(), _state()
    rp, rm, rv, re, rs = p.cpu().numpy().astype(np.float64), np.zeros(n), np.zeros(n), ema.cpu().numpy().astype(np.float64), R.fresh_state()
    for k, host in enumerate(grads):
        g = torch.from_numpy(host).to(_dev())
        _guard(g, st, 1.0, max_norm, 1)
        _adam(p, g, m, v, ema, st)
        rp, rm, rv, re, rs = R.guarded_step(rp, host, rm, rv, re, rs, LR, B1, B2, EPS, ALPHA, 1.0, max_norm, True, coef_to_f32=True)
        _guard(g, st_idle, 1.0, float("inf"), 1)
        _adam(idle[0], g, idle[1], idle[2], idle[3], st_idle)
        _lib.check(_lib.lib().tld_train_adam_ema(None, _p(plain[0]), _p(g), _p(plain[1]), _p(plain[2]), _p(plain[3]), n, LR, B1, B2, EPS, k + 1, ALPHA, 1.0,
                                                 _stream()), "tld_train_adam_ema")
    h = _head(st)
    assert h[R.T] == 2 and h[R.COEF] < 1 and abs(h[R.COEF] - rs[R.COEF]) <= 1e-12 * rs[R.COEF]
    assert abs(h[R.BC1] - rs[R.BC1]) <= 1e-15 and abs(h[R.BC2] - rs[R.BC2]) <= 1e-15
    ep, ee = np.abs(p.cpu().numpy() - rp).max(), np.abs(ema.cpu().numpy() - re).max()
    ip, ie = float((idle[0] - plain[0]).abs().max()), float((idle[3] - plain[3]).abs().max())
    print(f"n={n} off={off}: vs float64 params {ep:.2e} ema {ee:.2e}; idle guard vs plain kernel params {ip:.2e} ema {ie:.2e} (bound {UPDATE_TOL})")
    assert ep <= UPDATE_TOL and ee <= UPDATE_TOL
    assert _head(st_idle)[R.COEF] == 1.0 and ip <= UPDATE_TOL and ie <= UPDATE_TOL
    assert float((p - torch.from_numpy(p0.astype(np.float32)).to(_dev())).abs().max()) > 1e-4          # the steps were taken
    for full in (pf, mf, vf, ef):
        assert _sentinels_intact(full, n, off)


# ---- through Trainer: the tiny g15 model at batch 4 ------------------------------------------------------------------------------------------
def _batches(count, batch=4, seed=21):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        x = torch.randn(batch, 4, 32, 32, generator=gen) * 0.8
        y = torch.randn(batch, 768, generator=gen) * 0.5
        nl = torch.rand(batch, generator=gen) * 0.9 + 0.05
        noise = torch.randn(batch, 4, 32, 32, generator=gen)
        out.append((nl.view(-1, 1, 1, 1) * noise + (1 - nl.view(-1, 1, 1, 1)) * x, nl, y, x))
    return out


def _tiny(**kw):
    from transformer_latent_diffusion_amd import TrainConfig
    _, cfg, sd = _g15()
    kw.setdefault("use_graph", False)
    kw.setdefault("max_batch", 4)
    return _trainer(cfg, sd, train_cfg=TrainConfig(lr=3e-4, alpha=0.999, batch_size=kw["max_batch"]), **kw)


def _vectors(tr):
    return tr.params, tr.exp_avg, tr.exp_avg_sq, tr.ema


def _same_bits(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(_vectors(a), _vectors(b)))


def test_trainer_reports_the_norm_and_clips_like_the_reference():
    (batch,) = _batches(1)
    probe = _tiny()
    probe.forward_backward(*batch)
    norm0 = float(torch.cat([v.reshape(-1) for v in probe.grad_dict().values()]).double().norm())
    tr = _tiny(max_grad_norm=0.5 * norm0)
    tr.forward_backward(*batch)
    g = tr.grads.cpu().numpy()
    p0, e0 = tr.params.cpu().numpy(), tr.ema.cpu().numpy()
    tr.optimizer_step()
    view = tr.grad_norm
    assert view.dim() == 0 and view.is_cuda and view.dtype == torch.float64
    ref = float(R.grad_norm(g, 1.0))
    stats = tr.optimizer_stats()
    print(f"trainer grad norm {float(view):.17g} ref {ref:.17g}; coef {stats['clip_coef']:.6f}")
    assert abs(float(view) - ref) <= 1e-12 * ref and stats["grad_norm"] == float(view)
    assert abs(ref - norm0) <= 1e-12 * norm0                                  # the backward is bit-reproducible
    assert 0.49 < stats["clip_coef"] < 0.5 and stats["applied_steps"] == 1 and stats["skipped_steps"] == 0 and stats["last_skipped"] is False
    rp, _, _, re, _ = R.guarded_step(p0, g, np.zeros_like(p0), np.zeros_like(p0), e0, R.fresh_state(), LR, B1, B2, EPS, ALPHA, 1.0, 0.5 * norm0, False,
                                     coef_to_f32=True)
    ep, ee = np.abs(tr.params.cpu().numpy() - rp).max(), np.abs(tr.ema.cpu().numpy() - re).max()
    print(f"post-step params {ep:.2e} ema {ee:.2e}")
    assert ep <= UPDATE_TOL and ee <= UPDATE_TOL and tr.step == 1


def test_trainer_skips_a_nan_step_bit_for_bit():
    good0, bad, good1 = _batches(3)
    a, b = _tiny(max_grad_norm=1.0, skip_nonfinite=True), _tiny(max_grad_norm=1.0, skip_nonfinite=True)
    a.forward_backward(*good0); a.optimizer_step()
    a.forward_backward(*bad)
    a.grads[a.numel // 3] = float("nan")
    a.optimizer_step()
    mid = a.optimizer_stats()
    assert mid["last_skipped"] is True and np.isnan(mid["grad_norm"]) and mid["applied_steps"] == 1
    a.forward_backward(*good1); a.optimizer_step()
    for batch in (good0, good1):
        b.forward_backward(*batch); b.optimizer_step()
    assert _same_bits(a, b)
    sa, sb = a.optimizer_stats(), b.optimizer_stats()
    assert sa["skipped_steps"] == 1 and sa["applied_steps"] == 2 and sa["last_skipped"] is False and a.step == 3
    assert sb["skipped_steps"] == 0 and sb["applied_steps"] == 2 and sa["grad_norm"] == sb["grad_norm"]


def test_trainer_norm_under_accumulation_is_the_norm_of_the_mean_gradient():
    """Two micro-batches of 4 against one batch of 8, at the gradient tolerance of test_gradient_accumulation_equals_one_large_batch (1e-5 relative L2:
    |norm a - norm b| <= |a - b|)."""
    (xn, nl, y, x), = _batches(1, batch=8)
    one, acc = _tiny(max_batch=8, skip_nonfinite=True), _tiny(max_batch=8, skip_nonfinite=True)
    one.forward_backward(xn, nl, y, x); one.optimizer_step()
    acc.forward_backward(xn[:4], nl[:4], y[:4], x[:4], last_micro_batch=False)
    acc.forward_backward(xn[4:], nl[4:], y[4:], x[4:]); acc.optimizer_step()
    n1, na = float(one.grad_norm), float(acc.grad_norm)
    print(f"norm of one batch of 8: {n1:.9g}; of two micro-batches of 4: {na:.9g}; relative difference {abs(na - n1) / n1:.2e}")
    assert n1 > 0 and abs(na - n1) <= 1e-5 * n1


def test_trainer_checkpoint_carries_the_applied_steps_and_resumes_bit_for_bit(tmp_path):
    good0, bad, good1, nxt = _batches(4)
    tr = _tiny(max_grad_norm=1.0, skip_nonfinite=True)
    tr.forward_backward(*good0); tr.optimizer_step()
    tr.forward_backward(*bad); tr.grads[5] = float("inf"); tr.optimizer_step()
    tr.forward_backward(*good1); tr.optimizer_step()
    ck = tr.checkpoint()
    stats = tr.optimizer_stats()
    assert stats["applied_steps"] == 2 and stats["skipped_steps"] == 1 and tr.step == 3
    assert {float(s["step"]) for s in ck["opt_state"]["state"].values()} == {2.0}
    path = str(tmp_path / "ck.pth")
    torch.save(ck, path)
    # the reference resumes with the EMA weights in the live model (tld/train.py:92-104): the run that goes on takes them too, and KEEPS its
    # optimizer state on the device; the resumed one rebuilds it from the checkpoint
    tr.load_state_dict(ck["model_ema"])
    tr2 = _tiny(max_grad_norm=1.0, skip_nonfinite=True).load_checkpoint(path)
    s2 = tr2.optimizer_stats()
    assert tr2.step == 2 and s2["applied_steps"] == 2 and s2["skipped_steps"] == 0 and s2["last_skipped"] is False
    h, h2 = _head(tr._opt_state), _head(tr2._opt_state)
    assert abs(h[R.BC1] - h2[R.BC1]) <= 1e-15 and abs(h[R.BC2] - h2[R.BC2]) <= 1e-15
    for t in (tr, tr2):
        t.forward_backward(*nxt); t.optimizer_step()
    assert _same_bits(tr, tr2)
    assert tr.optimizer_stats()["applied_steps"] == tr2.optimizer_stats()["applied_steps"] == 3


def test_trainer_guarded_graph_replay_equals_eager():
    def run(graph):
        tr = _tiny(max_grad_norm=0.05, skip_nonfinite=True, use_graph=graph)
        gen, rng = torch.Generator().manual_seed(5), np.random.default_rng(7)
        losses = []
        for _ in range(4):
            x = torch.randn(4, 4, 32, 32, generator=gen); y = torch.randn(4, 768, generator=gen)
            losses.append(float(tr.train_step(x, y, np_rng=rng, generator=gen)))
        return tr, losses, tr.optimizer_stats()

    e, le, se = run(False)
    g, lg, sg = run(True)
    assert e._graph is None and g._graph is not None
    assert le == lg and _same_bits(e, g) and se == sg and se["applied_steps"] == 4


_RANK = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from transformer_latent_diffusion_amd import DenoiserConfig, TrainConfig, Trainer
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = DenoiserConfig(image_size=32, n_channels=4)
tr = Trainer(cfg, TrainConfig(lr=3e-4), device=dev, init_seed=3, max_batch=4, max_grad_norm={max_norm!r}, skip_nonfinite=True)
g = torch.Generator().manual_seed(7)
x = torch.randn(4, 4, 32, 32, generator=g) * 0.8; y = torch.randn(4, 768, generator=g) * 0.5
nl = torch.tensor([0.1, 0.3, 0.6, 0.8]); noise = torch.randn(4, 4, 32, 32, generator=g)
xn = nl.view(-1, 1, 1, 1) * noise + (1 - nl.view(-1, 1, 1, 1)) * x
sl = slice(r * 4 // w, (r + 1) * 4 // w)
tr.forward_backward(xn[sl], nl[sl], y[sl], x[sl])
tr.optimizer_step()
torch.cuda.synchronize()
torch.save(dict(params=tr.params.cpu(), stats=tr.optimizer_stats()), {out!r} + f".{{w}}.{{r}}")
print("rank", r, "done")
"""


def test_two_ranks_clip_alike_and_like_one_process(tmp_path):
    """Launched and compared as test_two_ranks_average_gradients_like_one_process does, with its tolerance; the norm is taken after the all-reduce,
    so both ranks hold the same one, bit for bit."""
    import transformer_latent_diffusion_amd as T
    script = tmp_path / "rank.py"
    out = str(tmp_path / "params")
    script.write_text(_RANK.format(repo=REPO, out=out, max_norm=1e-3))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for w in (2, 1):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={w}", "--master-addr", "127.0.0.1",
                            "--master-port", "29567", str(script)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b, one = (torch.load(out + s, weights_only=False) for s in (".2.0", ".2.1", ".1.0"))
    assert torch.equal(a["params"], b["params"]) and a["stats"] == b["stats"]
    print("two ranks:", a["stats"], "one process:", one["stats"])
    assert a["stats"]["clip_coef"] < 1 and one["stats"]["clip_coef"] < 1 and a["stats"]["applied_steps"] == 1
    assert abs(a["stats"]["grad_norm"] - one["stats"]["grad_norm"]) <= 1e-5 * one["stats"]["grad_norm"]       # summation order only, as under accumulation
    base = torch.cat([torch.from_numpy(np.array(v)).reshape(-1) for k, v in T.weights.synth_state_dict(T.DenoiserConfig(image_size=32, n_channels=4), 3).items()
                      if "angular" not in k and "precomputed" not in k])
    da, d1 = a["params"] - base, one["params"] - base
    agree = (torch.sign(da) == torch.sign(d1)).float().mean().item()
    assert agree > 0.97, agree
    assert (da - d1).abs().max() <= 2 * 3e-4 + 1e-7


def test_unguarded_trainer_owns_no_state_and_has_no_stats():
    tr = _tiny()
    assert tr.guarded is False and tr._opt_state is None
    with pytest.raises(RuntimeError, match="not guarded"):
        tr.optimizer_stats()
    with pytest.raises(RuntimeError, match="not guarded"):
        tr.grad_norm
    (batch,) = _batches(1)
    tr.forward_backward(*batch); tr.optimizer_step()
    assert tr.step == 1 and tr._opt_state is None

"""CPU: the guarded optimizer step's float64 reference (tests/grad_guard_ref.py) against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam on float64 tensors, the skip rule against a hand-written sequence, and the refusals of tld_train_grad_guard, which come
before any HIP call and so need no GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import grad_guard_ref as R
from transformer_latent_diffusion_amd import _lib

LR, B1, B2, EPS, ALPHA = 3e-4, 0.9, 0.999, 1e-8, 0.999
N = 1000


def _vectors(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) * 0.05, [rng.standard_normal(N) * 1e-2 for _ in range(3)]


def _close(a, b, tag):
    a, b = np.asarray(a), np.asarray(b)
    assert np.array_equal(np.isnan(a), np.isnan(b)), tag
    ok = ~np.isnan(b)
    if ok.any():
        assert np.abs(a[ok] - b[ok]).max() <= 1e-12 * np.abs(b[ok]).max(), (tag, float(np.abs(a[ok] - b[ok]).max()))


@pytest.mark.parametrize("case", ["clipped", "unclipped", "nan_norm_skip_off"])
def test_reference_equals_torch_clip_grad_norm_and_adam_in_float64(case):
    """Three steps of clip_grad_norm_(max_norm) + Adam.step() + update_ema on float64 CPU tensors, 1e-12 relative."""
    p0, grads = _vectors(1)
    norms = [float(np.linalg.norm(g)) for g in grads]
    max_norm = 0.5 * min(norms) if case == "clipped" else 2.0 * max(norms)
    if case == "nan_norm_skip_off":
        grads[1] = grads[1].copy(); grads[1][17] = np.nan
    w = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([w], lr=LR, betas=(B1, B2), eps=EPS)
    e = torch.from_numpy(p0.copy())
    p, m, v, ema, st = p0.copy(), np.zeros(N), np.zeros(N), p0.copy(), R.fresh_state()
    for k, g in enumerate(grads):
        w.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([w], max_norm)
        opt.step()
        e.mul_(ALPHA).add_(w.detach(), alpha=1 - ALPHA)
        p, m, v, ema, st = R.guarded_step(p, g, m, v, ema, st, LR, B1, B2, EPS, ALPHA, 1.0, max_norm, False)
        _close(st[R.NORM], float(total), (case, k, "norm"))
        _close(st[R.COEF] * g, w.grad.numpy(), (case, k, "clipped gradient"))
        if case == "clipped":
            assert st[R.COEF] < 0.51
        elif case == "unclipped":
            assert st[R.COEF] == 1.0
        elif k == 1:
            assert np.isnan(st[R.COEF]) and np.isnan(st[R.NORM])          # error_if_nonfinite=False: the NaN goes through
        assert st[R.T] == k + 1 and st[R.SKIPPED] == 0 and st[R.LAST_SKIPPED] == 0
        state = opt.state[w]
        _close(p, w.detach().numpy(), (case, k, "params"))
        _close(m, state["exp_avg"].numpy(), (case, k, "exp_avg"))
        _close(v, state["exp_avg_sq"].numpy(), (case, k, "exp_avg_sq"))
        _close(ema, e.numpy(), (case, k, "ema"))
    if case == "nan_norm_skip_off":
        assert np.isnan(p).all()


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_skip_sequence_good_bad_good_equals_good_good(bad):
    """GradScaler semantics by hand: the bad step changes nothing and does not advance the bias correction."""
    p0, (g0, gbad, g1) = _vectors(2)
    gbad = gbad.copy(); gbad[N // 2] = bad

    def run(seq):
        p, m, v, ema, st = p0.copy(), np.zeros(N), np.zeros(N), p0.copy(), R.fresh_state()
        log = []
        for g in seq:
            p, m, v, ema, st = R.guarded_step(p, g, m, v, ema, st, LR, B1, B2, EPS, ALPHA, 1.0, 0.01, True)
            log.append(st.copy())
        return p, m, v, ema, st, log

    a, b = run([g0, gbad, g1]), run([g0, g1])
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    sa, sb, log = a[4], b[4], a[5]
    assert sa[R.T] == 2 and sa[R.SKIPPED] == 1 and sa[R.LAST_SKIPPED] == 0 and sb[R.SKIPPED] == 0
    assert sa[R.BC1] == sb[R.BC1] == 1 - B1 ** 2 and sa[R.BC2] == sb[R.BC2]
    mid = log[1]
    assert mid[R.LAST_SKIPPED] == 1 and mid[R.COEF] == 0 and not np.isfinite(mid[R.NORM])
    assert mid[R.T] == 1 and mid[R.BC1] == log[0][R.BC1] and mid[R.BC2] == log[0][R.BC2]


def test_no_clipping_values_of_max_norm():
    for mn in (None, 0.0, -1.0, np.inf):
        st = R.finalize(R.fresh_state(), 4.0, mn, False, B1, B2)
        assert st[R.COEF] == 1.0 and st[R.NORM] == 2.0 and st[R.T] == 1
    st = R.finalize(R.fresh_state(), 4.0, 1.0, False, B1, B2)
    assert st[R.COEF] == 1.0 / (2.0 + 1e-6)


def test_grad_guard_refuses_bad_arguments_without_a_gpu():
    """TLD_ERR_INVALID with a text, before any HIP call: null pointers, numel <= 0, NaN max_norm, misaligned grads / state."""
    L = _lib.lib()
    assert _lib.TRAIN_OPT_STATE_DOUBLES == 8 + 1024
    buf = np.zeros(64, dtype=np.float64)                    # never dereferenced: every call below is refused on its arguments alone
    base = (buf.ctypes.data + 15) & ~15
    g, st = C.c_void_p(base), C.c_void_p(base + 64)
    cases = {
        "null grads": (None, 8, 1.0, st),
        "null state": (g, 8, 1.0, None),
        "numel 0": (g, 0, 1.0, st),
        "numel < 0": (g, -3, 1.0, st),
        "nan max_norm": (g, 8, float("nan"), st),
        "grads 4 bytes off": (C.c_void_p(base + 4), 8, 1.0, st),
        "grads 8 bytes off": (C.c_void_p(base + 8), 8, 1.0, st),
        "state 4 bytes off": (g, 8, 1.0, C.c_void_p(base + 68)),
    }
    for tag, (gp, n, mn, sp) in cases.items():
        rc = L.tld_train_grad_guard(None, gp, n, 1.0, mn, 1, B1, B2, sp, None)
        assert rc == 1, (tag, rc)
        msg = L.tld_last_error()
        assert msg and b"grad guard" in msg, (tag, msg)
    assert L.tld_train_adam_ema_guarded(None, g, g, g, g, None, 8, LR, B1, B2, EPS, ALPHA, 1.0, None, None) == 1 and L.tld_last_error()


def test_trainer_takes_the_guard_keywords():
    from transformer_latent_diffusion_amd import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    assert isinstance(Trainer.grad_norm, property) and callable(Trainer.optimizer_stats)

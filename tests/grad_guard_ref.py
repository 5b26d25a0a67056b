"""Float64 numpy statement of the guarded optimizer step (include/tld_hip.h: tld_train_grad_guard / tld_train_adam_ema_guarded): the
global gradient norm, the finalize rule (clip_grad_norm_ coefficient, GradScaler's non-finite skip, Adam's count of APPLIED steps) and the
Adam + EMA update on the clipped gradient.  tests/test_grad_guard_host.py holds it against torch.nn.utils.clip_grad_norm_ +
torch.optim.Adam in float64; tests/test_gpu_grad_guard.py holds the kernels against it.  Nothing here is rounded to fp32 except where the
ABI itself takes a float: callers that compare with the device pass float-rounded scalars (``f32``)."""
import numpy as np

from transformer_latent_diffusion_amd._lib import TRAIN_OPT_STATE_DOUBLES

PARTS = TRAIN_OPT_STATE_DOUBLES - 8           # partial sums behind the eight head entries
T, SKIPPED, LAST_SKIPPED, NORM, COEF, BC1, BC2 = range(7)      # head indices of the state vector


def f32(x):
    """The double a C float argument carries."""
    return float(np.float32(x))


def fresh_state():
    return np.zeros(8, dtype=np.float64)


def sqsum(g, scale):
    """sum (g[i] * float(scale))^2 in float64 (the product of two fp32 values is exact there)."""
    x = np.asarray(g, dtype=np.float64) * np.float64(f32(scale))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float64(np.sum(x * x))


def grad_norm(g, scale=1.0):
    return np.sqrt(sqsum(g, scale))


def clips(max_norm):
    return max_norm is not None and max_norm > 0 and np.isfinite(max_norm)


def finalize(state, sumsq, max_norm, skip_nonfinite, b1, b2):
    """The finalize rule on the head of the state vector; returns the new head."""
    st = np.array(state, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        norm = np.sqrt(np.float64(sumsq))
    st[NORM] = norm
    st[7] = 0.0
    if skip_nonfinite and not np.isfinite(sumsq):
        st[SKIPPED] += 1; st[LAST_SKIPPED] = 1; st[COEF] = 0
        return st
    st[LAST_SKIPPED] = 0
    st[T] += 1
    c = np.float64(max_norm if max_norm is not None else 0.0) / (norm + 1e-6)
    st[COEF] = (1.0 if c > 1 else c) if clips(max_norm) else 1.0
    st[BC1] = 1.0 - np.float64(b1) ** st[T]
    st[BC2] = 1.0 - np.float64(b2) ** st[T]
    return st


def guarded_step(p, g, m, v, ema, state, lr, b1, b2, eps, alpha, scale=1.0, max_norm=None, skip_nonfinite=False, coef_to_f32=False):
    """One guarded step on float64 copies: returns (p, m, v, ema, state).  ema may be None.  coef_to_f32: round the coefficient to float
    before it multiplies the gradient, as the kernel does."""
    p, m, v = (np.array(a, dtype=np.float64) for a in (p, m, v))
    ema = None if ema is None else np.array(ema, dtype=np.float64)
    st = finalize(state, sqsum(g, scale), max_norm, skip_nonfinite, b1, b2)
    if st[LAST_SKIPPED]:
        return p, m, v, ema, st
    coef = f32(st[COEF]) if coef_to_f32 else st[COEF]
    with np.errstate(over="ignore", invalid="ignore"):
        gi = (np.asarray(g, dtype=np.float64) * np.float64(f32(scale))) * coef
        m = b1 * m + (1.0 - b1) * gi
        v = b2 * v + (1.0 - b2) * gi * gi
        denom = np.sqrt(v) / np.sqrt(st[BC2]) + eps
        p = p - (lr / st[BC1]) * (m / denom)
        if ema is not None:
            ema = ema * alpha + p * (1.0 - alpha)
    return p, m, v, ema, st

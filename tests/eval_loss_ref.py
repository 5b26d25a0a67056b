"""Numpy statement of the loss-by-noise-level accumulator (tld_train_loss_buckets): the serial loop over the samples.
The device kernel is held to it bit for bit (tests/test_gpu_eval_loss.py); tests/test_eval_loss_host.py holds it to hand-made cases."""
import numpy as np


def fresh_state(n):
    """All zeros = an empty accumulator: [0, n) sums, [n, 2n) counts, [2n] total sum, [2n + 1] rejected."""
    return np.zeros(2 * int(n) + 2, dtype=np.float64)


def bucket_index(level, n):
    """min(n - 1, floor((double)level * n)) of one fp32 level, or -1 when the level is outside [0, 1] (NaN included)."""
    l = np.float64(np.float32(level))
    if not (l >= 0.0 and l <= 1.0):
        return -1
    return min(int(n) - 1, int(np.floor(l * np.float64(n))))


def accumulate(state, sample_loss, noise_level, n):
    """One call: returns the new state; sample_loss float64 [batch], noise_level float32 [batch]."""
    st = np.array(state, dtype=np.float64)
    loss = np.asarray(sample_loss, dtype=np.float64).reshape(-1)
    lev = np.asarray(noise_level, dtype=np.float32).reshape(-1)
    assert st.size == 2 * n + 2 and loss.size == lev.size
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(loss.size):
            k = bucket_index(lev[b], n)
            if k < 0:
                st[2 * n + 1] += 1.0
                continue
            st[k] = st[k] + loss[b]
            st[n + k] += 1.0
            st[2 * n] = st[2 * n] + loss[b]
    return st


def readout(state, n):
    """(loss, bucket_loss with NaN where a count is 0, bucket_count, rejected)"""
    st = np.asarray(state, dtype=np.float64)
    cnt = st[n:2 * n]
    with np.errstate(invalid="ignore", divide="ignore"):
        return st[2 * n] / cnt.sum(), np.where(cnt > 0, st[:n] / cnt, np.nan), cnt, st[2 * n + 1]


def edge_levels(n):
    """The fp32 levels every accumulator test includes: 0, 1, 1 - 2^-24, every bin edge k / n, and the three kinds of rejected level."""
    edges = (np.arange(n + 1, dtype=np.float64) / n).astype(np.float32)
    return np.concatenate([np.array([0.0, 1.0, 1.0 - 2.0 ** -24], dtype=np.float32), edges, np.array([-0.25, np.nan, 1.5], dtype=np.float32)])

"""A numpy statement of the device batch preparation (include/tld_hip.h: tld_train_prepare_batch), for
tests/test_batch_prep_host.py and tests/test_gpu_batch_prep.py.  Integer parts (Philox, the uniform conversions, the mask, the gather) are exact
and compared with ==; the Beta draw follows the kernel's algorithm with numpy's own log / cos, so it agrees to rounding, not in every bit."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
STREAM_NOISE, STREAM_LEVEL, STREAM_MASK = 0, 1, 2
LEVEL_SLOTS, GAMMA_TRIES = 64, 16
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (uint32, broadcastable) -> [..., 4] uint32.  Salmon et al., SC'11."""
    ctr = np.asarray(ctr, dtype=np.uint32)
    key = np.asarray(key, dtype=np.uint32)
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c = [np.broadcast_to(ctr[..., i], shape).astype(np.uint64) for i in range(4)]
    k0 = np.broadcast_to(key[..., 0], shape).astype(np.uint64)
    k1 = np.broadcast_to(key[..., 1], shape).astype(np.uint64)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK32]
        k0, k1 = (k0 + np.uint64(W0)) & MASK32, (k1 + np.uint64(W1)) & MASK32
    return np.stack(c, axis=-1).astype(np.uint32)


def batch_philox(seed, step, replica, stream, c0):
    """The draw at counter (c0, 4 replica + stream, step_lo, step_hi) under the key (seed_lo, seed_hi); c0: array -> [n, 4]."""
    c0 = np.asarray(c0, dtype=np.uint64)
    assert (c0 < (1 << 32)).all()
    ctr = np.empty(c0.shape + (4,), dtype=np.uint32)
    ctr[..., 0] = c0
    ctr[..., 1] = (4 * int(replica) + stream) & 0xFFFFFFFF
    ctr[..., 2] = int(step) & 0xFFFFFFFF
    ctr[..., 3] = (int(step) >> 32) & 0xFFFFFFFF
    return philox4x32_10(ctr, np.array([int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF], dtype=np.uint32))


def uniform24_open(r):
    """((r >> 8) + 0.5) 2^-24 with ONE fp32 addition and one fp32 product, in (0, 1]."""
    return ((np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform24_open_complement(r):
    """(2^24 - (r >> 8) - 0.5) 2^-24 in fp32: 1 - u, exact for r >> 8 >= 2^23."""
    k = np.asarray(r, dtype=np.uint32) >> np.uint32(8)
    return ((np.uint32(1 << 24) - k).astype(np.float32) - np.float32(0.5)) * np.float32(2.0 ** -24)


def uniform24(r):
    """float(r >> 8) 2^-24 in [0, 1), exact."""
    return (np.asarray(r, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniform53_open(hi, lo):
    k = ((np.asarray(hi, dtype=np.uint64) << np.uint64(32)) | np.asarray(lo, dtype=np.uint64)) >> np.uint64(11)
    return (k.astype(np.float64) + 0.5) * 2.0 ** -53


def uniform32_open(r):
    return (np.asarray(r, dtype=np.uint32).astype(np.float64) + 0.5) * 2.0 ** -32


def noise_words(seed, step, replica, n_elems):
    """Philox words of the flat noise elements [0, n_elems): [ceil(n / 4), 4]."""
    return batch_philox(seed, step, replica, STREAM_NOISE, np.arange((n_elems + 3) // 4, dtype=np.uint64))


def noise_f64(seed, step, replica, n_elems):
    """Box-Muller in float64 on the kernel's Philox words: elements 4 c0 .. 4 c0 + 3 from (r0, r1) and (r2, r3), u = ((r >> 8) + 0.5) 2^-24 unrounded."""
    w = noise_words(seed, step, replica, n_elems)
    u = ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24
    out = np.empty((w.shape[0], 4), dtype=np.float64)
    for h in range(2):
        rad = np.sqrt(-2.0 * np.log(u[:, 2 * h]))
        out[:, 2 * h] = rad * np.cos(2.0 * np.pi * u[:, 2 * h + 1])
        out[:, 2 * h + 1] = rad * np.sin(2.0 * np.pi * u[:, 2 * h + 1])
    return out.reshape(-1)[:n_elems]


def label_mask(seed, step, replica, batch, p):
    b = np.arange(batch, dtype=np.uint64)
    w = batch_philox(seed, step, replica, STREAM_MASK, b >> np.uint64(2))
    return uniform24(w[np.arange(batch), (b & np.uint64(3)).astype(np.int64)]) < np.float32(p)


def _log_gamma_draw(shape, base, seed, step, replica, batch):
    boost = shape < 1.0
    a1 = shape + 1.0 if boost else shape
    d = a1 - 1.0 / 3.0
    c = 1.0 / np.sqrt(9.0 * d)
    c0 = LEVEL_SLOTS * np.arange(batch, dtype=np.uint64) + np.uint64(base)
    g = np.full(batch, d)
    done = np.zeros(batch, dtype=bool)
    for j in range(GAMMA_TRIES):
        w = batch_philox(seed, step, replica, STREAM_LEVEL, c0 + np.uint64(j))
        x = np.sqrt(-2.0 * np.log(uniform53_open(w[:, 0], w[:, 1]))) * np.cos(2.0 * np.pi * uniform32_open(w[:, 2]))
        v = 1.0 + c * x
        ok = v > 0.0
        v3 = np.where(ok, v, 1.0) ** 3
        accept = ok & (np.log(uniform32_open(w[:, 3])) < 0.5 * x * x + d - d * v3 + d * np.log(v3)) & ~done
        g = np.where(accept, d * v3, g)
        done |= accept
    lg = np.log(g)
    if boost:
        w = batch_philox(seed, step, replica, STREAM_LEVEL, c0 + np.uint64(GAMMA_TRIES))
        lg = lg + np.log(uniform53_open(w[:, 0], w[:, 1])) / shape
    return lg, done


def noise_level(seed, step, replica, batch, a, b, return_exhausted=False):
    """Beta(a, b) per sample as 1 / (1 + exp(ln Gamma_b - ln Gamma_a)), the Gammas by Marsaglia-Tsang with at most GAMMA_TRIES attempts."""
    lx, dx = _log_gamma_draw(float(a), 0, seed, step, replica, batch)
    ly, dy = _log_gamma_draw(float(b), LEVEL_SLOTS // 2, seed, step, replica, batch)
    with np.errstate(over="ignore"):
        nl = 1.0 / (1.0 + np.exp(ly - lx))
    return (nl, int((~dx).sum() + (~dy).sum())) if return_exhausted else nl


def gather(latents, labels, idx, table=None, scale=8.0):
    """target, label (before the mask) and the bad-index count for numpy sources: codes through the table, floats through one fp32 division."""
    idx = np.asarray(idx, dtype=np.int64)
    bad = (idx < 0) | (idx >= latents.shape[0])
    rows = np.where(bad, 0, idx)
    lat = latents[rows].reshape(len(idx), -1)
    target = table[lat.astype(np.int64)] if latents.dtype == np.uint8 else lat.astype(np.float32) / np.float32(scale)
    return target.astype(np.float32), labels[rows].astype(np.float32), int(bad.sum())

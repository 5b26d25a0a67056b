"""The plan of one sampler call and the bytes of its staged upload, restated in numpy from the contracts of include/tld_hip.h (tld_sample ...
tld_sample_requests_shaped), the flavour table of DESIGN.md section 7.17 and the layouts of the three row structs -- not from
csrc/tld_sample_plan.h, which tests/test_sample_plan_host.py holds against this file.

A call is a ``Call``: the records in the engine's order, the host arrays as float32 / uint64 numpy arrays or None, and the engine's two facts."""
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np

UNIFORM, REQUESTS, GUIDED, STOCHASTIC, SHAPED = range(5)
FILL = 0xCD                      # what the staging buffer holds before the fill: the bytes of an alignment gap keep it
ROW_CAP = 1024

STEP_ROW = np.dtype([("g", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("c1", "<f4"), ("c2", "<f4"), ("s_next", "<f4"), ("final", "<i4")])
NOISE_ROW = np.dtype([("e", "<f4"), ("key_lo", "<u4"), ("key_hi", "<u4"), ("reserved", "<u4")])
assert STEP_ROW.itemsize == 32 and NOISE_ROW.itemsize == 16

# (entry, a guidance table is present) -> (slots, noise, shape, skip follows the engine, batch check per step)
FLAVOUR = {
    (UNIFORM, False): (False, False, False, False, False),
    (REQUESTS, False): (False, False, False, False, False),
    (GUIDED, True): (True, False, False, True, True),
    (STOCHASTIC, True): (True, True, False, True, True),
    (STOCHASTIC, False): (True, True, False, False, False),
    (SHAPED, True): (True, True, True, True, True),
    (SHAPED, False): (True, True, True, False, False),
}


@dataclass
class Call:
    entry: int
    B: int
    n_max: int
    stride: int                                  # 1: a record and a table per request; 0: one of each for the whole batch
    records: Optional[Sequence[Tuple[int, float, float, int]]]     # (n_levels, class_guidance, start_mix, has_negative)
    coeffs: Optional[np.ndarray]                 # float32 [B or 1][n_max][6]
    guidance: Optional[np.ndarray] = None        # float32 [B][n_max]
    noise_coeff: Optional[np.ndarray] = None     # float32 [B][n_max]
    noise_keys: Optional[np.ndarray] = None      # uint64 [B]
    shape: Optional[np.ndarray] = None           # float32 [B][4]
    has_mask: bool = False
    has_init: bool = False
    has_neg_labels: bool = False
    guidance_skip: bool = True
    max_batch: int = 64


def plan(c: Call) -> dict:
    """Everything the engine decides before it launches, for a call that is refused nowhere."""
    B, n_max = c.B, c.n_max
    recs = [c.records[b * c.stride] for b in range(B)]
    counts = np.array([r[0] for r in recs])
    slots_f, noise_f, shape_f, skip_f, _ = FLAVOUR[(c.entry, c.guidance is not None)]
    skip = skip_f and c.guidance_skip
    g = np.zeros((B, n_max), np.float32)
    for b, r in enumerate(recs):
        g[b] = np.float32(r[1]) if c.guidance is None else c.guidance[b]
    running = counts[None, :] > np.arange(n_max)[:, None]                       # [step][request]
    Bi = running.sum(1)
    assert all(running[i, :Bi[i]].all() for i in range(n_max)), "the running requests are a prefix"
    has_unc = running & (~np.bool_(skip) | (g.T != np.float32(1.0))) if slots_f else running
    slot = np.where(has_unc, np.cumsum(has_unc, 1) - 1, -1)
    slot = np.where(running, slot, -2)                                           # -2: not running, no statement
    U = has_unc.sum(1)
    neutral = np.ones(B, bool) if c.shape is None else (c.shape == np.array([1, 0, 0, 0], np.float32)).all(1)
    beta = np.zeros(B, np.float32) if c.shape is None else c.shape[:, 2]
    shaped_at = has_unc & ~neutral[None, :] & (g.T != np.float32(1.0)) if shape_f else np.zeros_like(running)
    # the conditioning rows
    if c.stride:
        seen, sig = {}, []
        idx = np.zeros((n_max, B), np.int64)
        for i in range(n_max):
            for b in range(Bi[i]):
                key = c.coeffs[b, i, 0].tobytes()
                if key not in seen:
                    seen[key] = len(sig)
                    sig.append(c.coeffs[b, i, 0])
                idx[i, b] = seen[key]
        sig = np.array(sig, np.float32)
    else:
        sig = c.coeffs[0, :, 0].astype(np.float32)
        idx = np.repeat(np.arange(n_max)[:, None], B, 1)
    n_neg = sum(1 for r in recs if r[3])
    tabB = B if c.stride else 1
    per = 3 if slots_f else 2
    mb = Bi + U
    step_rows_off = np.concatenate([[0], np.cumsum(per * mb)[:-1]])
    cells = n_max * tabB
    mix_off = cells * 32
    rows_off = mix_off + 4 * tabB
    rows_end = rows_off + 4 * per * int(mb.sum())
    noise_off = -(-rows_end // 16) * 16
    shape_off = noise_off + 16 * cells
    up_bytes = shape_off + 16 * tabB if shape_f else shape_off if noise_f else rows_end
    return dict(slots=int(slots_f), noise=int(noise_f), shape=int(shape_f), skip=int(skip), B=B, n_max=n_max, stride=c.stride, tabB=tabB, per=per,
                Tn=len(sig), n_neg=n_neg, T=len(sig) + B + 1 + n_neg, rows_cond=int(Bi.sum()), rows_uncond=int(U.sum()),
                any_mix=int(any(np.float32(r[2]) < 1 for r in recs)), any_shape=int(shaped_at.any()),
                any_mom=int((shaped_at & (beta != 0)[None, :]).any()), mix_off=mix_off, rows_off=rows_off, noise_off=noise_off, shape_off=shape_off,
                up_bytes=up_bytes, stage_bytes=up_bytes + 4 * len(sig), Bi=Bi.tolist(), U=U.tolist(), mb=mb.tolist(),
                step_rows_off=step_rows_off.tolist(), stats=shaped_at.any(1).astype(int).tolist(), slot=slot.reshape(-1).tolist(),
                sig=sig.view(np.uint32).tolist(), noise_idx=idx.reshape(-1).tolist(), _g=g)


def upload(c: Call, p: dict) -> bytes:
    """The staging buffer after the fill: the upload and, behind it, the sigmas."""
    B, n_max, tabB, Tn = c.B, c.n_max, p["tabB"], p["Tn"]
    buf = np.full(p["stage_bytes"], FILL, np.uint8)
    g, slot, idx = p["_g"], np.array(p["slot"]).reshape(n_max, B), np.array(p["noise_idx"]).reshape(n_max, B)
    # the step rows: zero past a request's levels; the next level's sigma except on the final forward, which carries the flag; the slots
    # flavour packs (slot + 1) << 1 into the flag's word
    tab = np.zeros((n_max, tabB), STEP_ROW)
    for b in range(tabB):
        n, co = c.records[b][0], c.coeffs[b]
        for i in range(n):
            tab[i, b] = (g[b, i], co[i, 1], co[i, 2], co[i, 3], co[i, 4], co[i, 5], co[i + 1, 0] if i + 1 < n else 0.0, int(i == n - 1))
            if p["slots"]:
                tab["final"][i, b] |= (int(slot[i, b]) + 1) << 1
    buf[:p["mix_off"]] = np.frombuffer(tab.tobytes(), np.uint8)
    mix = np.array([c.records[b][2] for b in range(tabB)], "<f4")
    buf[p["mix_off"]:p["rows_off"]] = np.frombuffer(mix.tobytes(), np.uint8)
    # the int tables: per step the model samples are the running requests, then the unconditional samples in slot order
    zero_row = Tn + B
    neg_row, k = [], 0
    for b in range(B):
        has = c.records[b * c.stride][3]
        neg_row.append(zero_row + 1 + k if has else zero_row)
        k += 1 if has else 0
    ints = []
    for i in range(n_max):
        Bi = p["Bi"][i]
        unc = sorted((int(slot[i, b]), b) for b in range(Bi) if slot[i, b] >= 0)
        assert [s for s, _ in unc] == list(range(p["U"][i]))
        src = list(range(Bi)) + [b for _, b in unc]
        ints += [int(idx[i, b]) for b in src]
        ints += [Tn + b for b in range(Bi)] + [neg_row[b] for _, b in unc]
        if p["slots"]:
            ints += src
    rows = np.array(ints, "<i4")
    buf[p["rows_off"]:p["rows_off"] + 4 * len(rows)] = np.frombuffer(rows.tobytes(), np.uint8)
    if p["noise"]:
        nt = np.zeros((n_max, tabB), NOISE_ROW)
        for b in range(tabB):
            key = 0 if c.noise_keys is None else int(c.noise_keys[b])
            nt["key_lo"][:, b], nt["key_hi"][:, b] = key & 0xFFFFFFFF, key >> 32
            if c.noise_coeff is not None:
                inner = c.records[b][0] - 1
                nt["e"][:inner, b] = c.noise_coeff[b, :inner]
        buf[p["noise_off"]:p["shape_off"]] = np.frombuffer(nt.tobytes(), np.uint8)
    if p["shape"]:
        buf[p["shape_off"]:p["up_bytes"]] = np.frombuffer(np.ascontiguousarray(c.shape[:tabB], "<f4").tobytes(), np.uint8)
    buf[p["up_bytes"]:] = np.frombuffer(np.array(p["sig"], "<u4").tobytes(), np.uint8)
    return buf.tobytes()

"""A numpy restatement of csrc/tld_session_plan.h: the slot and conditioning-row tables of a sampler session and the bytes of every step's upload.

Written from the header's rules, not from its code: rows lowest-free-first, sigma rows shared by float32 bit pattern and reference counted, live
requests in ascending slot order, the unconditional samples compacted in that order.  tests/test_session_plan_host.py holds the header to it byte
for byte (tests/host/session_plan_main.cpp)."""
import math

import numpy as np

F = np.float32
OK, INVALID = 0, 1
ROW_CAP = 1024
FREE, ZERO, LABEL, SIGMA = 0, 1, 2, 3


def bits(v):
    return int(np.array([v], F).view(np.uint32)[0])


class Request:
    """One request as tld_session_admit takes it; every array may be None (a null pointer)."""

    def __init__(self, coeffs, g=3.0, has_negative=0, has_neg_label=None, guidance=None, noise_coeff=None, key=None, n_levels=None, reserved=0):
        self.coeffs = None if coeffs is None else np.ascontiguousarray(coeffs, F).reshape(-1, 6)
        self.n_levels = (0 if coeffs is None else self.coeffs.shape[0]) if n_levels is None else n_levels
        self.g = F(g)
        self.has_negative = int(has_negative)
        self.has_neg_label = bool(has_negative) if has_neg_label is None else bool(has_neg_label)
        self.guidance = None if guidance is None else np.ascontiguousarray(guidance, F)
        self.noise_coeff = None if noise_coeff is None else np.ascontiguousarray(noise_coeff, F)
        self.key = key
        self.reserved = reserved

    def guided_at(self, i):
        return self.guidance[i] if self.guidance is not None else self.g


def fmt_g(v):
    """printf's %g of a float promoted to double."""
    return "%g" % float(v)


def open_check(slots, cond_rows, max_batch):
    if slots < 1:
        return [INVALID, f"a session needs at least one slot (have {slots})"]
    if 2 * slots > max_batch:
        return [INVALID, f"a session of {slots} slots needs max_batch >= {2 * slots} (have {max_batch})"]
    if cond_rows < 3 or cond_rows > ROW_CAP:
        return [INVALID, f"cond_rows = {cond_rows}: a session takes 3 .. {ROW_CAP} conditioning rows"]
    return [OK, ""]


def request_check(r):
    if r is None or r.coeffs is None:
        return [INVALID, "null argument"]
    if r.reserved != 0:
        return [INVALID, f"request: reserved = {r.reserved}: expected 0"]
    if (r.noise_coeff is None) != (r.key is None):
        return [INVALID, "noise_coeff and noise_key come together (both NULL: no noise)"]
    if r.n_levels < 2:
        return [INVALID, f"request: need at least two noise levels (have {r.n_levels})"]
    if r.guidance is None and not math.isfinite(float(r.g)):
        return [INVALID, "request: class_guidance is not finite"]
    if r.guidance is not None:
        for i in range(r.n_levels):
            if not math.isfinite(float(r.guidance[i])):
                return [INVALID, f"request: guidance of forward {i} is not finite"]
    if r.has_negative and not r.has_neg_label:
        return [INVALID, "request: has_negative without neg_label"]
    if r.noise_coeff is not None:
        for i in range(r.n_levels):
            en = r.noise_coeff[i]
            if not (math.isfinite(float(en)) and en >= 0):
                return [INVALID, f"request: noise_coeff of forward {i} is {fmt_g(en)}: expected finite and >= 0"]
            if i == r.n_levels - 1 and en != 0:
                return [INVALID, f"request: noise_coeff of its final forward {i} is {fmt_g(en)}: the final prediction takes no noise, expected 0"]
    return [OK, ""]


class Session:
    def __init__(self, slots, cond_rows, skip=True):
        self.slots, self.cond_rows, self.skip = slots, cond_rows, bool(skip)
        self.req = [None] * slots            # the live request of a slot
        self.next = [-1] * slots
        self.label = [-1] * slots
        self.neg = [-1] * slots
        self.sig = [[] for _ in range(slots)]
        self.kind = [FREE] * cond_rows
        self.ref = [0] * cond_rows
        self.bits = [0] * cond_rows
        self.kind[0] = ZERO
        self.steps = self.rows_cond = self.rows_uncond = 0

    # ---- what the driver prints as the state
    @property
    def live(self):
        return sum(r is not None for r in self.req)

    @property
    def rows_used(self):
        return sum(k != FREE for k in self.kind)

    def state(self):
        sig = []
        for s in range(self.slots):
            sig += [-1] + list(self.sig[s])
        return dict(live=self.live, rows_used=self.rows_used, steps=self.steps, rows_cond=self.rows_cond, rows_uncond=self.rows_uncond,
                    sig_rows=sum(k == SIGMA for k in self.kind), row_kind=list(self.kind), row_ref=list(self.ref), row_bits=list(self.bits),
                    slot_live=[int(r is not None) for r in self.req], slot_next=list(self.next), slot_label=list(self.label), slot_neg=list(self.neg),
                    slot_sig=sig)

    def _take(self, kind):
        row = self.kind.index(FREE)           # lowest free first
        self.kind[row], self.ref[row] = kind, 1
        return row

    def _release(self, row):
        self.ref[row] -= 1
        if self.ref[row] == 0:
            self.kind[row], self.bits[row] = FREE, 0

    def admit(self, r):
        """(refusal, slot, new_sigma as a flat [row, bits, ...] list, label_row, neg_row) of a request that passed request_check."""
        sig_bits = [bits(r.coeffs[i, 0]) for i in range(r.n_levels)]
        distinct = list(dict.fromkeys(sig_bits))
        own = len(distinct) + 1 + (1 if r.has_negative else 0)
        if own > self.cond_rows - 1:
            return ([INVALID, f"the request needs {own} conditioning rows ({len(distinct)} distinct noise levels + 1 label + {1 if r.has_negative else 0} "
                              f"negative label): the session has {self.cond_rows - 1} beside the zero row"], -1, [], -1, -1)
        have = {self.bits[row]: row for row in range(self.cond_rows) if self.kind[row] == SIGMA}
        fresh = 1 + (1 if r.has_negative else 0) + sum(b not in have for b in distinct)
        free_slots = [s for s in range(self.slots) if self.req[s] is None]
        if not free_slots or fresh > self.cond_rows - self.rows_used:
            return ([OK, ""], -1, [], -1, -1)
        s = free_slots[0]
        new_sigma = []
        for b in distinct:
            if b in have:
                self.ref[have[b]] += 1
                continue
            row = self._take(SIGMA)
            self.bits[row] = b
            have[b] = row
            new_sigma += [row, b]
        self.req[s], self.next[s] = r, 0
        self.sig[s] = [have[b] for b in sig_bits]
        self.label[s] = self._take(LABEL)
        self.neg[s] = self._take(LABEL) if r.has_negative else -1
        return ([OK, ""], s, new_sigma, self.label[s], self.neg[s])

    def step(self):
        """The step's sizes, finished slots and upload bytes; then the requests move on and the finished ones leave."""
        liveslots = [s for s in range(self.slots) if self.req[s] is not None]
        if not liveslots:
            return dict(Bi=0, U=0, mb=0, noise=0, noise_off=0, ints_off=0, up_bytes=0, finished=[], bytes="")
        Bi = len(liveslots)
        noise = any(self.req[s].noise_coeff is not None for s in liveslots)
        uslot, U = [], 0
        for s in liveslots:
            r, i = self.req[s], self.next[s]
            has = not (self.skip and r.guidance is not None) or r.guided_at(i) != F(1.0)
            uslot.append(U if has else -1)
            U += has
        mb = Bi + U
        rows = np.zeros((Bi, 8), np.uint32)
        nrows = np.zeros((Bi, 4), np.uint32)
        nr, lr, sr, es = (np.zeros(mb, np.int32) for _ in range(4))
        finished = []
        for b, s in enumerate(liveslots):
            r, i = self.req[s], self.next[s]
            final = i == r.n_levels - 1
            co = r.coeffs[i]
            vals = np.array([r.guided_at(i), co[1], co[2], co[3], co[4], co[5], F(0) if final else r.coeffs[i + 1, 0]], F)
            rows[b, :7] = vals.view(np.uint32)
            rows[b, 7] = np.uint32(int(final) | (uslot[b] + 1) << 1)
            on = r.noise_coeff is not None and not final
            key = 0 if r.key is None else int(r.key)
            nrows[b] = [bits(r.noise_coeff[i]) if on else 0, key & 0xFFFFFFFF, key >> 32, i]
            nr[b], lr[b], sr[b], es[b] = self.sig[s][i], self.label[s], b, s
            if uslot[b] >= 0:
                k = Bi + uslot[b]
                nr[k], lr[k], sr[k], es[k] = nr[b], (self.neg[s] if self.neg[s] >= 0 else 0), b, s
            if final:
                finished.append(s)
        parts = [rows.tobytes()] + ([nrows.tobytes()] if noise else []) + [np.array(liveslots, np.int32).tobytes(), nr.tobytes(), lr.tobytes(), sr.tobytes(),
                                                                              es.tobytes()]
        blob = b"".join(parts)
        noise_off = 32 * Bi
        ints_off = noise_off + (16 * Bi if noise else 0)
        assert len(blob) == ints_off + 4 * (Bi + 4 * mb)
        self.rows_cond += Bi
        self.rows_uncond += U
        self.steps += 1
        for s in liveslots:
            self.next[s] += 1
        for s in finished:
            for row in sorted(set(self.sig[s])):
                self._release(row)
            self._release(self.label[s])
            if self.neg[s] >= 0:
                self._release(self.neg[s])
            self.req[s], self.next[s], self.label[s], self.neg[s], self.sig[s] = None, -1, -1, -1, []
        return dict(Bi=Bi, U=U, mb=mb, noise=int(noise), noise_off=noise_off, ints_off=ints_off, up_bytes=len(blob), finished=finished, bytes=blob.hex())

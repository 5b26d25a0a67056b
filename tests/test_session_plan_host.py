"""CPU: the host side of a sampler session -- csrc/tld_session_plan.h through tests/host/session_plan_main.cpp, built by the
host compiler plain and under AddressSanitizer + UBSan, against the numpy restatement (tests/session_plan_ref.py) byte for byte on every emitted
table, against the rows sample_plan_fill writes for each request alone (made in the driver with the existing header), and against the invariants of
the slot and row tables; and every refusal that needs no device, with its code and text."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import session_plan_ref as R
from transformer_latent_diffusion_amd import schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _table(n, exponent=1, plus=True, eta=0.0):
    levels = schedule.noise_schedule(n, exponent)
    if eta > 0.0:
        co, e = schedule.step_coefficients(levels, plus, eta)
        return np.ascontiguousarray(co, F), np.ascontiguousarray(e, F)
    return np.ascontiguousarray(schedule.step_coefficients(levels, plus), F), None


def _bits(a):
    return " ".join(f"{int(v):x}" for v in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32))


def _admit_line(r):
    arr = lambda tag, a: f"{tag} -1" if a is None else f"{tag} {np.asarray(a).size} {_bits(a)}"
    key = "K -1" if r.key is None else f"K 1 {int(r.key):x}"
    return " ".join(["admit", str(r.n_levels), _bits([r.g]), str(r.has_negative), str(int(r.has_neg_label)), str(r.reserved), arr("C", r.coeffs),
                     arr("G", r.guidance), arr("E", r.noise_coeff), key])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver, built twice (run directly, nothing preloaded); ``run(lines)`` returns each build's parsed output."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    tmp = tmp_path_factory.mktemp("session_plan")
    src = [os.path.join(REPO, "tests", "host", "session_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"session_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exes[tag]], check=True)
    count = [0]

    def run(lines):
        count[0] += 1
        path = tmp / f"script_{count[0]}.txt"
        path.write_text("\n".join(lines) + "\n")
        out = {}
        for tag, exe in exes.items():
            p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert p.returncode == 0, (tag, p.returncode, p.stderr[-2000:])
            out[tag] = [json.loads(l) for l in p.stdout.splitlines()]
            assert len(out[tag]) == len(lines), (tag, len(out[tag]), len(lines))
        return out

    return run


# ---- randomized admit / step sequences -------------------------------------------------------------------------------------------------------------
def _random_request(rng):
    n = int(rng.integers(2, 13))
    eta = float(rng.choice([0.0, 0.0, 0.5, 1.0]))
    expo = int(rng.choice([1, 1, 2]))        # (the stochastic table needs strictly decreasing levels: exponent 1 there)
    co, e = _table(n, exponent=1 if eta > 0.0 else expo, plus=bool(rng.integers(0, 2)), eta=eta)
    kind = int(rng.integers(0, 3))
    guidance = None
    g = float(rng.choice([1.0, 3.0, 4.5, 6.0]))
    if kind == 1:                            # a table with runs of exact 1.0 (an interval)
        lo, hi = sorted(rng.integers(0, n + 1, size=2))
        guidance = np.full(n, 1.0, F)
        guidance[lo:hi] = g
    elif kind == 2:                          # a table with scattered 1.0
        guidance = np.where(rng.random(n) < 0.4, 1.0, g).astype(F)
    neg = int(rng.random() < 0.35)
    key = None if e is None else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
    return R.Request(co, g=g, has_negative=neg, guidance=guidance, noise_coeff=e, key=key)


def _sequence(seed, slots, cond_rows, skip, min_steps=200):
    """(script lines, the restatement's answer per line): admissions at random between steps for min_steps steps, then steps until the last request left."""
    rng = np.random.default_rng(seed)
    S = R.Session(slots, cond_rows, skip)
    lines, want = [f"open {slots} {cond_rows} {int(skip)} {2 * slots}"], [dict(op="open", check=[0, ""])]

    def do_step():
        lines.append("step")
        want.append(dict(op="step", **S.step(), **S.state()))

    steps = 0
    while steps < min_steps:
        for _ in range(int(rng.integers(0, 3))):
            r = _random_request(rng)
            lines.append(_admit_line(r))
            bad = R.request_check(r)
            assert bad == [0, ""], bad
            free = S.live < slots
            full, slot, new_sigma, label_row, neg_row = S.admit(r)
            w = dict(op="admit", check=bad, admit=full, slot=slot, label_row=label_row, neg_row=neg_row, new_sigma=new_sigma, free_slot=free)
            if not full[0]:
                w.update(S.state())
            want.append(w)
        do_step()
        steps += 1
    while S.live:
        do_step()
    return lines, want, S


SEQUENCES = [(1, 1, 16, True), (2, 2, 20, True), (3, 3, 24, False), (4, 4, 30, True), (5, 5, 26, True), (6, 6, 40, False), (7, 7, 34, True), (8, 8, 38, True)]


@pytest.mark.parametrize("seed,slots,cond_rows,skip", SEQUENCES, ids=[f"slots{s[1]}_rows{s[2]}" for s in SEQUENCES])
def test_random_sequences_against_the_restatement_and_the_solo_plans(driver, seed, slots, cond_rows, skip):
    lines, want, S = _sequence(seed, slots, cond_rows, skip)
    got = driver(lines)
    n_steps = sum(l == "step" for l in lines)
    assert n_steps >= 200
    deferred_rows = deferred_slots = never = admitted = 0
    for tag in ("plain", "san"):
        assert len(got[tag]) == len(want)
        for k, (g, w) in enumerate(zip(got[tag], want)):
            for key, val in w.items():
                if key == "free_slot":
                    continue
                assert g[key] == val, (tag, k, lines[k][:60], key, g[key], val)
            if w["op"] == "open" or ("admit" in w and w["admit"][0]):
                continue
            # ---- the invariants, on the header's own state
            kind, ref, live = g["row_kind"], g["row_ref"], g["slot_live"]
            sig_of = []
            flat, cur = g["slot_sig"], None
            for v in flat:
                if v == -1:
                    cur = []
                    sig_of.append(cur)
                else:
                    cur.append(v)
            assert len(sig_of) == slots
            owned = [r for s in range(slots) if live[s] for r in (g["slot_label"][s], g["slot_neg"][s]) if r >= 0]
            assert len(owned) == len(set(owned)) and all(kind[r] == R.LABEL and ref[r] == 1 for r in owned), (tag, k, "a label row is owned twice")
            assert kind[0] == R.ZERO and 0 not in owned
            for row in range(1, cond_rows):
                need = sum(1 for s in range(slots) if live[s] and row in sig_of[s])
                if kind[row] == R.SIGMA:
                    assert ref[row] == need and need > 0, (tag, k, row, ref[row], need)
                elif kind[row] == R.LABEL:
                    assert row in owned and need == 0
                else:
                    assert ref[row] == 0 and need == 0 and row not in owned
            sig_bits = [g["row_bits"][row] for row in range(cond_rows) if kind[row] == R.SIGMA]
            assert len(sig_bits) == len(set(sig_bits)) == g["sig_rows"], (tag, k, "a sigma has two rows")
            assert g["rows_used"] == sum(x != R.FREE for x in kind) and g["live"] == sum(live)
            for s in range(slots):
                if not live[s]:
                    assert g["slot_label"][s] == -1 and g["slot_neg"][s] == -1 and not sig_of[s] and g["slot_next"][s] == -1
            if w["op"] == "step":
                assert g["tail"] == 1, (tag, k, "a byte behind up_bytes was written")
                assert g["solo"] == 1, (tag, k, "an emitted row differs from the row of the request alone")
                assert g["mb"] <= 2 * slots and g["Bi"] <= slots
            elif tag == "plain":
                if g["slot"] >= 0:
                    admitted += 1
                    assert g["solo_planned"] == 1
        last = got[tag][-1]
        assert last["live"] == 0 and last["rows_used"] == 1 and not any(last["row_kind"][1:]) and not any(last["slot_live"]), "rows or slots left after the last request"
        assert last["rows_cond"] == last["solo_rows_cond"] and last["rows_uncond"] == last["solo_rows_uncond"], \
            (last["rows_cond"], last["solo_rows_cond"], last["rows_uncond"], last["solo_rows_uncond"])
    for w in want:                           # what kinds of "no room now" the sequence met
        if w["op"] != "admit":
            continue
        if w["admit"][0]:
            never += 1
        elif w["slot"] < 0:
            deferred_rows += w["free_slot"]
            deferred_slots += not w["free_slot"]
    print(f"slots {slots}, cond_rows {cond_rows}: {n_steps} steps, {admitted} admitted, deferred for a slot {deferred_slots}, for rows {deferred_rows}, never fit {never}")
    assert admitted > 20 and deferred_slots + deferred_rows > 0


def test_row_exhaustion_and_slot_exhaustion_both_happen(driver):
    """Across the sequences above both kinds of "no room now" must occur; this one makes each on purpose and holds the answer: slot -1, TLD_OK."""
    t4, _ = _table(4)
    t5, _ = _table(5, 2)
    lines = ["open 2 10 1 4", _admit_line(R.Request(t4)), _admit_line(R.Request(t5)), "open 3 32 1 6"] + [_admit_line(R.Request(t4))] * 4
    got = driver(lines)
    for tag in ("plain", "san"):
        g = got[tag]
        assert g[1]["slot"] == 0 and g[1]["rows_used"] == 6                       # zero + 4 sigmas + label
        assert g[2]["admit"] == [0, ""] and g[2]["slot"] == -1 and g[2]["rows_used"] == 6 and g[2]["live"] == 1      # 5 sigmas + label > 4 free rows
        assert [x["slot"] for x in g[4:8]] == [0, 1, 2, -1] and g[7]["admit"] == [0, ""]                            # no free slot
        assert g[7]["rows_used"] == 1 + 4 + 3 and g[6]["new_sigma"] == []                                           # the schedule's rows are shared


# ---- the refusals that need no device --------------------------------------------------------------------------------------------------------------
def _refusals():
    t3, e3 = _table(3, eta=1.0)
    nan, inf = F(np.nan), F(np.inf)
    bad_e = e3.copy(); bad_e[1] = -0.5
    nan_e = e3.copy(); nan_e[0] = nan
    last_e = e3.copy(); last_e[2] = 0.25
    return {
        "null coeffs": (R.Request(None, n_levels=3), "check", "null argument"),
        "reserved": (R.Request(t3, reserved=7), "check", "request: reserved = 7: expected 0"),
        "table without a key": (R.Request(t3, noise_coeff=e3), "check", "noise_coeff and noise_key come together (both NULL: no noise)"),
        "key without a table": (R.Request(t3, key=5), "check", "noise_coeff and noise_key come together (both NULL: no noise)"),
        "one level": (R.Request(t3, n_levels=1), "check", "request: need at least two noise levels (have 1)"),
        "no level": (R.Request(t3, n_levels=0), "check", "request: need at least two noise levels (have 0)"),
        "guidance nan": (R.Request(t3, g=nan), "check", "request: class_guidance is not finite"),
        "guidance inf": (R.Request(t3, g=inf), "check", "request: class_guidance is not finite"),
        "table nan": (R.Request(t3, guidance=[3.0, nan, 1.0]), "check", "request: guidance of forward 1 is not finite"),
        "table inf at the end": (R.Request(t3, guidance=[3.0, 1.0, -inf]), "check", "request: guidance of forward 2 is not finite"),
        "negative without its label": (R.Request(t3, has_negative=1, has_neg_label=False), "check", "request: has_negative without neg_label"),
        "noise_coeff negative": (R.Request(t3, noise_coeff=bad_e, key=1), "check", "request: noise_coeff of forward 1 is -0.5: expected finite and >= 0"),
        "noise_coeff nan": (R.Request(t3, noise_coeff=nan_e, key=1), "check", "request: noise_coeff of forward 0 is nan: expected finite and >= 0"),
        "noise_coeff on the final forward": (R.Request(t3, noise_coeff=last_e, key=1), "check",
                                             "request: noise_coeff of its final forward 2 is 0.25: the final prediction takes no noise, expected 0"),
        "never fits": (R.Request(_table(7)[0], has_negative=1), "admit",
                       "the request needs 9 conditioning rows (7 distinct noise levels + 1 label + 1 negative label): the session has 7 beside the zero row"),
    }


def test_every_device_free_refusal_with_code_and_text(driver):
    cases = _refusals()
    lines = ["open 2 8 1 4"] + [_admit_line(r) for r, _, _ in cases.values()]
    # a guidance table makes the scalar irrelevant: a NaN record value beside a finite table is fine
    fine = R.Request(_table(3)[0], g=F(np.nan), guidance=[1.0, 2.0, 1.0])
    lines.append(_admit_line(fine))
    got = driver(lines)
    for tag in ("plain", "san"):
        out = got[tag]
        assert out[0] == dict(op="open", check=[0, ""])
        for (name, (r, stage, text)), g in zip(cases.items(), out[1:]):
            if stage == "check":
                assert g["check"] == [1, text] == R.request_check(r), (tag, name, g["check"])
                assert "admit" not in g
            else:
                assert g["check"] == [0, ""] and g["admit"] == [1, text] and g["slot"] == -1, (tag, name, g)
                assert R.Session(2, 8).admit(r)[0] == [1, text]
                assert g["live"] == 0 and g["rows_used"] == 1, "a refused request took rows"
        assert out[-1]["check"] == [0, ""] and out[-1]["admit"] == [0, ""] and out[-1]["slot"] == 0


def test_open_refusals(driver):
    cases = [("open 0 8 1 64", "a session needs at least one slot (have 0)"), ("open 5 8 1 9", "a session of 5 slots needs max_batch >= 10 (have 9)"),
             ("open 2 2 1 64", "cond_rows = 2: a session takes 3 .. 1024 conditioning rows"),
             ("open 2 1025 1 64", "cond_rows = 1025: a session takes 3 .. 1024 conditioning rows"), ("open 32 1024 1 64", ""), ("open 1 3 1 2", "")]
    got = driver([c for c, _ in cases])
    for tag in ("plain", "san"):
        for (line, text), g in zip(cases, got[tag]):
            assert g["check"] == [1 if text else 0, text], (tag, line, g)
            toks = [int(t) for t in line.split()[1:]]
            assert R.open_check(toks[0], toks[1], toks[3]) == g["check"]


def test_through_the_library_without_a_device():
    """The session entries before any HIP call: a null engine or session is TLD_ERR_INVALID; the record checks come before the session is looked at;
    and tld_session_open asks for finalized weights (TLD_ERR_STATE) before it looks at the sizes (the engine itself needs a device to exist, so that
    order is read from the source here and the status held on the device by tests/test_gpu_session.py)."""
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    err = lambda: L.tld_last_error().decode()
    out = C.c_void_p()
    assert L.tld_session_open(None, 2, 8, 0.0, 0.0, None, C.byref(out)) == 1 and err() == "null argument" and not out.value
    assert L.tld_session_open(None, 2, 8, 0.0, 0.0, None, None) == 1
    t3 = _table(3)[0]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    slot = C.c_int32(7)
    rq = _lib.TldSessionRequest(3, 3.0, 0, 0, fp(t3), None, None, None, C.c_void_p(16), C.c_void_p(16), None)
    assert L.tld_session_admit(None, C.byref(rq), None, C.byref(slot)) == 1 and err() == "null argument"
    rq.n_levels = 1
    assert L.tld_session_admit(None, C.byref(rq), None, C.byref(slot)) == 1 and err() == "request: need at least two noise levels (have 1)"
    assert L.tld_session_admit(None, None, None, C.byref(slot)) == 1 and err() == "null argument"
    n = C.c_int32(0)
    done = (C.c_int32 * 4)()
    assert L.tld_session_step(None, None, done, 4, C.byref(n)) == 1 and err() == "null argument"
    assert L.tld_session_latent(None, 0, C.byref(out)) == 1 and L.tld_session_copy_latent(None, 0, None, None) == 1
    assert L.tld_session_stats(None, None) == 1 and L.tld_session_close(None) == 0
    src = open(os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc", "tld_engine.hip")).read()
    body = src[src.index("int tld_session_open("):]
    order = [body.index(s) for s in ("!e || !out", "!e->finalized", "e->session", "session_open_check(", "hipStreamIsCapturing", "new tld_session")]
    assert order == sorted(order)
    # while a session is open the engine's other entries are refused: each holds the test
    for entry in ("int sample_requests(", "int tld_denoiser_forward(", "int tld_engine_refresh_weights("):
        fn = src[src.index(entry):]
        assert "if (e->session) return fail(TLD_ERR_STATE" in fn[:fn.index("\n}\n")], entry


def test_the_cap_is_the_python_layers_cap():
    assert schedule.REQUEST_ROW_CAP == R.ROW_CAP == 1024

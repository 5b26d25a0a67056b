"""CPU: the host side of every sampler call -- csrc/tld_sample_plan.h through tests/host/sample_plan_main.cpp, built by
the host compiler plain and under AddressSanitizer + UBSan, against the numpy restatement of the plan and of the upload bytes
(tests/sample_plan_ref.py) and against the planning helpers of schedule.py; and every refusal of the six entries that needs no device, with its
code, its full text and its precedence."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import sample_plan_ref as R
from transformer_latent_diffusion_amd import schedule

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NEUTRAL, RESCALE, APG = (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.7), (0.0, 2.5, -0.5, 0.0)


def _table(n, exponent=1, plus=True):
    return np.ascontiguousarray(schedule.step_coefficients(schedule.noise_schedule(n, exponent), plus), dtype=F)


def _last_bit(tab, row):
    t = tab.copy()
    t[row, 0] = np.nextafter(t[row, 0], F(2.0))
    return t


def requests_call(entry, tabs, g=None, mix=None, neg=None, gsteps=None, ecs=None, keys=None, shape=None, skip=True, max_batch=64, has_mask=False):
    """A call of one of the four requests entries from per-request lists in the CALLER's order, sorted as denoiser.py sorts them."""
    B = len(tabs)
    counts = [t.shape[0] for t in tabs]
    order = schedule.request_order(counts)
    n_max = counts[order[0]]
    g, mix, neg = g or [3.0] * B, mix or [1.0] * B, neg or [0] * B
    table, gtab, etab = np.zeros((B, n_max, 6), F), None, None
    for k, b in enumerate(order):
        table[k, :counts[b]] = tabs[b]
    if gsteps is not None:
        gtab = np.zeros((B, n_max), F)
        for k, b in enumerate(order):
            gtab[k, :counts[b]] = gsteps[b]
    if ecs is not None:
        etab = np.zeros((B, n_max), F)
        for k, b in enumerate(order):
            etab[k, :counts[b]] = ecs[b]
    c = R.Call(entry, B, n_max, 1, [(counts[b], g[b], mix[b], neg[b]) for b in order], table, gtab, etab,
               None if keys is None else np.array([keys[b] for b in order], np.uint64), None if shape is None else np.array([shape[b] for b in order], F),
               has_mask=has_mask, has_init=has_mask or any(v < 1 for v in mix), has_neg_labels=any(neg), guidance_skip=skip, max_batch=max_batch)
    c.order, c.tabs = order, [tabs[b] for b in order]
    return c


def uniform_call(B, tab, g=3.0, mix=1.0, has_mask=False, has_init=False, max_batch=64):
    return R.Call(R.UNIFORM, B, tab.shape[0], 0, [(tab.shape[0], g, mix, 0)], tab[None].copy(), has_mask=has_mask, has_init=has_init, max_batch=max_batch)


def _bits(a):
    return " ".join(f"{int(v):x}" for v in np.ascontiguousarray(a, F).reshape(-1).view(np.uint32))


def _line(name, c):
    arr = lambda tag, a: f"{tag} -1" if a is None else f"{tag} {np.asarray(a).size} {_bits(a)}"
    recs = "R -1" if c.records is None else f"R {len(c.records)} " + " ".join(f"{r[0]} {_bits([r[1]])} {_bits([r[2]])} {r[3]}" for r in c.records)
    keys = "K -1" if c.noise_keys is None else f"K {len(c.noise_keys)} " + " ".join(f"{int(k):x}" for k in c.noise_keys)
    return " ".join([name, str(c.entry), str(c.B), str(c.n_max), str(c.stride), str(int(c.has_mask)), str(int(c.has_init)), str(int(c.has_neg_labels)),
                     str(int(c.guidance_skip)), str(c.max_batch), recs, arr("C", c.coeffs), arr("G", c.guidance), arr("E", c.noise_coeff), keys,
                     arr("S", c.shape)])


# ---- the calls that are planned -----------------------------------------------------------------------------------------------------------------
def _plan_cases():
    t2, t3, t4, t5 = _table(2), _table(3), _table(4), _table(5)
    t4b, t3d = _table(4, 2), _table(3, 1, False)
    cases = {}
    shapes = {"B1": [t2], "B3": [t4, t2, t4], "B5": [t3, t5, t2, t3, t2], "B2": [t3, t4b], "B4": [t4, t4b, t3d, t4]}
    for tag, tabs in shapes.items():
        cases[f"requests {tag}"] = requests_call(R.REQUESTS, tabs, g=[1.0 + b for b in range(len(tabs))])
    cases["uniform B3"] = uniform_call(3, t4)
    cases["uniform B1 from, mix"] = uniform_call(1, t3, mix=0.5, has_mask=True, has_init=True)
    # guidance tables: exact 1.0 at some steps, at all steps of one request, at a whole step (U_i = 0); skip on and off
    g5 = [[3.0, 1.0, 2.0], [1.0, 1.0, 4.0, 1.0, 2.0], [1.0, 1.0], [2.0, 1.0, 1.0], [2.5, 1.0]]
    g3 = [[1.0, 2.0, 1.0, 3.0], [1.0, 4.0], [1.0, 1.0, 2.0, 1.0]]
    for skip in (True, False):
        cases[f"guided B5 skip={skip}"] = requests_call(R.GUIDED, shapes["B5"], gsteps=g5, skip=skip)
        cases[f"guided B3 whole step at 1 skip={skip}"] = requests_call(R.GUIDED, shapes["B3"], gsteps=g3, skip=skip)
        cases[f"guided B1 all 1 skip={skip}"] = requests_call(R.GUIDED, [t2], gsteps=[[1.0, 1.0]], skip=skip)
    # negative labels with runs and gaps, start mixes, a mask
    cases["requests negatives 0 1 1 0 1"] = requests_call(R.REQUESTS, [t3] * 5, neg=[0, 1, 1, 0, 1])
    cases["guided negatives, mixes, mask"] = requests_call(R.GUIDED, shapes["B5"], gsteps=g5, neg=[1, 0, 1, 1, 0], mix=[1.0, 0.5, 1.0, 0.25, 1.0], has_mask=True)
    # duplicate sigmas across requests; a sigma that differs in the last bit only
    cases["sigmas shared"] = requests_call(R.REQUESTS, [t4, t4, t3, t4])
    cases["sigma last bit"] = requests_call(R.REQUESTS, [t4, _last_bit(t4, 2), t4])
    # the stochastic entry with and without a table
    e5 = [np.r_[np.full(t.shape[0] - 1, 0.125 * (b + 1), F), F(0)] for b, t in enumerate(shapes["B5"])]
    k5 = [0x0123456789ABCDEF, 7, 1 << 63, (1 << 64) - 1, 0]
    cases["stochastic table"] = requests_call(R.STOCHASTIC, shapes["B5"], gsteps=g5, ecs=e5, keys=k5)
    cases["stochastic no table, g = 1 record"] = requests_call(R.STOCHASTIC, shapes["B5"], g=[1.0, 2.0, 1.0, 3.0, 1.0], ecs=e5, keys=k5)
    cases["stochastic no table, skip off"] = requests_call(R.STOCHASTIC, shapes["B3"], ecs=[np.array([0.5, 0.25, 0.125, 0], F), np.array([0.5, 0], F), np.zeros(4, F)], keys=k5[:3], skip=False)
    # the shaped entry: noise present or absent, rows all neutral, mixed, with beta != 0, and guided steps at 1.0 only
    for noise in (True, False):
        kw = dict(ecs=e5, keys=k5) if noise else {}
        cases[f"shaped neutral noise={noise}"] = requests_call(R.SHAPED, shapes["B5"], gsteps=g5, shape=[NEUTRAL] * 5, **kw)
        cases[f"shaped mixed noise={noise}"] = requests_call(R.SHAPED, shapes["B5"], gsteps=g5, shape=[NEUTRAL, RESCALE, NEUTRAL, RESCALE, NEUTRAL], **kw)
        cases[f"shaped beta noise={noise}"] = requests_call(R.SHAPED, shapes["B5"], gsteps=g5, shape=[RESCALE, APG, NEUTRAL, NEUTRAL, RESCALE], **kw)
        cases[f"shaped no table noise={noise}"] = requests_call(R.SHAPED, shapes["B3"], g=[2.0, 1.0, 3.0], shape=[APG, APG, NEUTRAL],
                                                                **(dict(ecs=[np.zeros(4, F), np.zeros(2, F), np.zeros(4, F)], keys=k5[:3]) if noise else {}))
    for skip in (True, False):
        cases[f"shaped guided at 1.0 only skip={skip}"] = requests_call(R.SHAPED, [t3, t2], gsteps=[[1.0, 1.0, 1.0], [1.0, 1.0]], shape=[APG, RESCALE], skip=skip)
    # the cap, exactly: 1024 rows are accepted
    cases["row cap 1024"] = _cap_call(1024)
    return cases


def _cap_call(rows):
    """B = 11 requests of 92 levels with distinct sigmas everywhere: 11 x 92 + 11 + 1 = 1024 rows; one negative label makes 1025."""
    B, n = 11, 92
    tabs = []
    for b in range(B):
        t = np.zeros((n, 6), F)
        t[:, 0] = (F(1.0) + np.arange(b * n, (b + 1) * n, dtype=F) / F(4096)).astype(F)
        t[:, 1:] = 1.0
        tabs.append(t)
    return requests_call(R.REQUESTS, tabs, neg=[0] * (B - 1) + [rows - 1024])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver, built twice (run directly, nothing preloaded); ``run(cases)`` returns each build's parsed output."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    tmp = tmp_path_factory.mktemp("sample_plan")
    src = [os.path.join(REPO, "tests", "host", "sample_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"sample_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exes[tag]], check=True)

    def run(cases):
        path = tmp / f"cases_{len(os.listdir(tmp))}.txt"
        path.write_text("".join(_line(f"case{k}", c) + "\n" for k, c in enumerate(cases.values())))
        outs = []
        for tag, exe in exes.items():
            r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
            outs.append([json.loads(ln) for ln in r.stdout.splitlines()])
        assert outs[0] == outs[1], "the sanitizer build answers differently"
        assert len(outs[0]) == len(cases)
        return dict(zip(cases, outs[0]))

    return run


@pytest.fixture(scope="module")
def planned(driver):
    cases = _plan_cases()
    return cases, driver(cases)


def test_plan_and_upload_bytes_equal_the_restatement(planned):
    cases, got = planned
    for name, c in cases.items():
        out = got[name]
        assert out["check"] == [0, ""] and out["plan"] == [0, ""], (name, out)
        want = R.plan(c)
        for key, v in want.items():
            if not key.startswith("_"):
                assert out[key] == v, (name, key, out[key], v)
        assert bytes.fromhex(out["bytes"]) == R.upload(c, want), name
        # 16-byte rows sit on 16-byte offsets; the ints and the sigmas on 4
        assert out["noise_off"] % 16 == 0 and out["shape_off"] % 16 == 0 and out["mix_off"] % 4 == 0 and out["rows_off"] % 4 == 0 and out["up_bytes"] % 4 == 0, name
        assert out["stage_bytes"] == out["up_bytes"] + 4 * out["Tn"] and len(out["bytes"]) == 2 * out["stage_bytes"], name


def test_plan_equals_the_planning_helpers_of_schedule(planned):
    """active_prefix / guided_rows / distinct_sigma_rows / request_cond_rows on the same requests, sorted by request_order."""
    cases, got = planned
    for name, c in cases.items():
        out = got[name]
        if c.stride == 0:
            assert out["Bi"] == [c.B] * c.n_max and out["U"] == out["Bi"] and out["Tn"] == c.n_max and out["T"] == c.n_max + c.B + 1, name
            continue
        counts = [r[0] for r in c.records]
        assert counts == sorted(counts, reverse=True) and out["Bi"] == schedule.active_prefix(counts), name
        if out["slots"]:
            tables = [c.guidance[b, :n] if c.guidance is not None else np.full(n, c.records[b][1], F) for b, n in enumerate(counts)]
            U, slots, _ = schedule.guided_rows(counts, tables, bool(out["skip"]))
            slot = np.array(out["slot"]).reshape(c.n_max, c.B)
            assert out["U"] == U and all(slot[i, :len(s)].tolist() == s for i, s in enumerate(slots)), name
        else:
            assert out["U"] == out["Bi"], name
        assert out["mb"] == [a + b for a, b in zip(out["Bi"], out["U"])], name
        assert out["rows_cond"] == sum(counts) and out["rows_uncond"] == sum(out["U"]), name
        sig, rows = schedule.distinct_sigma_rows(c.tabs)
        idx = np.array(out["noise_idx"]).reshape(c.n_max, c.B)
        assert out["sig"] == sig.view(np.uint32).tolist() and all(idx[:n, b].tolist() == rows[b] for b, n in enumerate(counts)), name
        assert out["T"] == schedule.request_cond_rows(c.tabs, sum(r[3] for r in c.records)), name


def test_flavours_follow_the_table_of_the_design(planned):
    cases, got = planned
    seen = set()
    for name, c in cases.items():
        out, key = got[name], (c.entry, c.guidance is not None)
        slots, noise, shape, skip, _ = R.FLAVOUR[key]
        assert (out["slots"], out["noise"], out["shape"], out["skip"]) == (int(slots), int(noise), int(shape), int(skip and c.guidance_skip)), name
        assert out["per"] == (3 if slots else 2), name
        seen.add(key)
    assert seen == set(R.FLAVOUR), "a row of the table that no case reaches"
    assert got["shaped guided at 1.0 only skip=True"]["any_shape"] == 0 and got["shaped guided at 1.0 only skip=False"]["any_shape"] == 0
    assert got["shaped guided at 1.0 only skip=False"]["stats"] == [0, 0, 0] and got["shaped guided at 1.0 only skip=False"]["U"] == [2, 2, 1]
    assert got["shaped beta noise=True"]["any_mom"] == 1 and got["shaped mixed noise=False"]["any_mom"] == 0 and got["shaped mixed noise=False"]["any_shape"] == 1
    assert got["shaped neutral noise=True"]["any_shape"] == 0 and got["guided B3 whole step at 1 skip=True"]["U"][0] == 0
    assert got["sigma last bit"]["Tn"] == 5 and got["sigmas shared"]["Tn"] == len({v.tobytes() for t in cases["sigmas shared"].tabs for v in t[:, 0]}) < 15


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------------
def _refusal_cases():
    t3, t4 = _table(3), _table(4)
    nan, inf = float("nan"), float("inf")
    ok = lambda entry=R.REQUESTS, **kw: requests_call(entry, [t4, t3, t3], **kw)
    e3 = [np.array([0.5, 0.25, 0.125, 0], F), np.array([0.5, 0.25, 0], F), np.array([0.5, 0.25, 0], F)]
    g3 = [[2.0, 1.0, 2.0, 1.0], [2.0, 2.0, 1.0], [1.0, 1.0, 1.0]]
    sto = lambda **kw: ok(R.STOCHASTIC, **{**dict(ecs=e3, keys=[1, 2, 3]), **kw})
    shp = lambda **kw: ok(R.SHAPED, **{**dict(shape=[NEUTRAL, RESCALE, APG]), **kw})

    def edit(c, **kw):
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def rec(c, b, **kw):
        r = dict(zip(("n", "g", "mix", "neg"), c.records[b]))
        r.update(kw)
        c.records[b] = (r["n"], r["g"], r["mix"], r["neg"])
        return c

    def at(c, field, index, v):
        getattr(c, field)[index] = v
        return c

    cases = {
        # tld_sample_from, run_uniform
        "from start_mix 0": (uniform_call(2, t3, mix=0.0, has_init=True), "check", "start_mix 0 outside (0, 1]"),
        "from start_mix nan": (uniform_call(2, t3, mix=nan, has_init=True), "check", "start_mix nan outside (0, 1]"),
        "from start_mix 1.5": (uniform_call(2, t3, mix=1.5, has_init=True), "check", "start_mix 1.5 outside (0, 1]"),
        "from mask without init": (uniform_call(2, t3, has_mask=True), "check", "init_latent is required with a mask or with start_mix < 1"),
        "from mix without init": (uniform_call(2, t3, mix=0.5), "check", "init_latent is required with a mask or with start_mix < 1"),
        "uniform batch 0": (uniform_call(0, t3), "plan", "sampler batch 0 needs max_batch >= 0 (have 64)"),
        "uniform batch over": (uniform_call(5, t3, max_batch=9), "plan", "sampler batch 5 needs max_batch >= 10 (have 9)"),
        "uniform one level": (edit(uniform_call(2, t3), n_max=1), "plan", "need at least two noise levels"),
        # tld_sample_requests_shaped's own
        "shaped null shape": (ok(R.SHAPED), "check", "null argument: shape"),
        "shaped coeff without keys": (shp(ecs=e3), "check", "noise_coeff and noise_keys come together (both NULL: no noise)"),
        "shaped keys without coeff": (shp(keys=[1, 2, 3]), "check", "noise_coeff and noise_keys come together (both NULL: no noise)"),
        "shaped batch 0": (edit(shp(), B=0), "check", "need positive sizes (batch 0, n_max 4)"),
        "shaped n_max 0": (edit(shp(), n_max=0), "check", "need positive sizes (batch 3, n_max 0)"),
        # sample_requests
        "null requests": (edit(ok(), records=None), "check", "null argument"),
        "null coeffs": (edit(ok(), coeffs=None), "check", "null argument"),
        "batch 0": (edit(ok(), B=0), "check", "null argument"),
        "guided null table": (ok(R.GUIDED), "check", "null argument"),
        "stochastic null coeff": (ok(R.STOCHASTIC, keys=[1, 2, 3]), "check", "null argument: noise_coeff"),
        "stochastic null keys": (ok(R.STOCHASTIC, ecs=e3), "check", "null argument: noise_keys"),
        "shape eta_par": (shp(shape=[NEUTRAL, (-1.0, 0.0, 0.0, 0.0), APG]), "check", "request 1: shape (-1, 0, 0, 0): bad eta_par (expected finite and >= 0)"),
        "shape norm_r": (shp(shape=[(1.0, inf, 0.0, 0.5), NEUTRAL, APG]), "check", "request 0: shape (1, inf, 0, 0.5): bad norm_r (expected finite and >= 0)"),
        "shape beta": (shp(shape=[NEUTRAL, NEUTRAL, (1.0, 0.0, 1.0, 0.0)]), "check", "request 2: shape (1, 0, 1, 0): bad beta (expected |beta| < 1)"),
        "shape phi": (shp(shape=[NEUTRAL, (1.0, 0.0, 0.0, 1.5), APG]), "check", "request 1: shape (1, 0, 0, 1.5): bad phi (expected inside [0, 1])"),
        "mask without init": (edit(ok(has_mask=True), has_init=False), "check", "init_latent is required with a mask"),
        "one level": (rec(ok(), 2, n=1), "check", "request 2: need at least two noise levels (have 1)"),
        "levels over n_max": (edit(ok(), n_max=3), "check", "request 0: 4 levels beside a coefficient table of n_max = 3"),
        "not ordered": (rec(rec(ok(), 1, n=2), 2, n=3), "check",
                        "request 2 has 3 levels after request 1 with 2: the records must be ordered by non-increasing n_levels"),
        "start_mix 0": (edit(rec(ok(), 1, mix=0.0), has_init=True), "check", "request 1: start_mix 0 outside (0, 1]"),
        "start_mix 2": (edit(rec(ok(), 0, mix=2.0), has_init=True), "check", "request 0: start_mix 2 outside (0, 1]"),
        "class_guidance inf": (rec(ok(), 1, g=inf), "check", "request 1: class_guidance is not finite"),
        "stochastic no table, class_guidance nan": (rec(sto(), 2, g=nan), "check", "request 2: class_guidance is not finite"),
        "guidance table nan": (at(ok(R.GUIDED, gsteps=g3), "guidance", (1, 2), nan), "check", "request 1: guidance of forward 2 is not finite"),
        "start_mix without init": (edit(ok(mix=[1.0, 0.5, 1.0]), has_init=False), "check", "request 1: init_latent is required with start_mix < 1"),
        "negative without labels": (edit(ok(neg=[0, 0, 1]), has_neg_labels=False), "check", "request 2: has_negative without neg_labels"),
        "noise_coeff negative": (at(sto(), "noise_coeff", (0, 1), -0.25), "check", "request 0: noise_coeff of forward 1 is -0.25: expected finite and >= 0"),
        "noise_coeff nan": (at(sto(gsteps=g3), "noise_coeff", (2, 0), nan), "check", "request 2: noise_coeff of forward 0 is nan: expected finite and >= 0"),
        "noise_coeff final": (at(sto(), "noise_coeff", (1, 2), 0.5), "check",
                              "request 1: noise_coeff of its final forward 2 is 0.5: the final prediction takes no noise, expected 0"),
        "shaped noise_coeff final": (at(shp(ecs=e3, keys=[1, 2, 3]), "noise_coeff", (0, 3), 0.5), "check",
                                     "request 0: noise_coeff of its final forward 3 is 0.5: the final prediction takes no noise, expected 0"),
        "n_max too large": (edit(requests_call(R.REQUESTS, [t3, t3]), n_max=4, coeffs=np.zeros((2, 4, 6), F)), "check", "n_max = 4, but the longest request has 3 levels"),
        "batch over": (ok(max_batch=5), "plan", "sampler batch 3 needs max_batch >= 6 (have 5)"),
        "stochastic no table batch over": (sto(max_batch=5), "plan", "sampler batch 3 needs max_batch >= 6 (have 5)"),
        "guided step over": (ok(R.GUIDED, gsteps=g3, max_batch=4), "plan", "step 0 runs 3 requests and 2 unconditional samples: needs max_batch >= 5 (have 4)"),
        "guided step over, skip off": (ok(R.GUIDED, gsteps=g3, max_batch=5, skip=False), "plan",
                                       "step 0 runs 3 requests and 3 unconditional samples: needs max_batch >= 6 (have 5)"),
        "guided later step over": (ok(R.GUIDED, gsteps=[[1.0, 2.0, 2.0, 2.0], [1.0, 2.0, 1.0], [1.0, 2.0, 1.0]], max_batch=5), "plan",
                                   "step 1 runs 3 requests and 3 unconditional samples: needs max_batch >= 6 (have 5)"),
        "row cap 1025": (_cap_call(1025), "plan",
                         "the call needs 1025 conditioning rows (1012 distinct noise levels + 11 labels + 1 + 1 negative labels): at most 1024"),
        # precedence: the earlier check wins
        "two faults: shape row before the records": (rec(shp(shape=[NEUTRAL, NEUTRAL, (1.0, 0.0, 1.0, 0.0)]), 0, mix=0.0), "check",
                                                     "request 2: shape (1, 0, 1, 0): bad beta (expected |beta| < 1)"),
        "two faults: request 0 before request 1": (rec(rec(ok(), 1, n=1), 0, g=nan), "check", "request 0: class_guidance is not finite"),
        "two faults: the records before max_batch": (rec(ok(max_batch=2), 2, n=1), "check", "request 2: need at least two noise levels (have 1)"),
        "two faults: max_batch before the row cap": (edit(_cap_call(1025), max_batch=21), "plan", "sampler batch 11 needs max_batch >= 22 (have 21)"),
    }
    return cases


def test_every_refusal_holds_its_code_text_and_precedence(driver):
    cases = _refusal_cases()
    got = driver({k: v[0] for k, v in cases.items()})
    for name, (_, stage, text) in cases.items():
        out = got[name]
        if stage == "plan":
            assert out["check"] == [0, ""], (name, out["check"])
        assert out[stage] == [1, text], (name, out[stage])
        assert "bytes" not in out, name
    # the uniform entries are checked for max_batch only after `finalized`, the requests entries' pointers only after the records: the .hip keeps both tests
    src = open(os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc", "tld_engine.hip")).read()
    body = src[src.index("int sample_requests("):]
    order = [body.index(s) for s in ("sample_call_check(call)", "!e || !ops.noise || !ops.labels || !ops.out_latent", "!e->finalized", "sample_plan(call, e->plan)",
                                     "run_sampler(e, e->plan")]
    assert order == sorted(order)


def test_the_cap_is_the_python_layers_cap():
    assert schedule.REQUEST_ROW_CAP == R.ROW_CAP == 1024
    hdr = open(os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc", "tld_sample_plan.h")).read()
    assert "constexpr int kMaxRequestCondRows = 1024;" in hdr
    for inc in [ln for ln in hdr.splitlines() if ln.startswith("#include \"")]:
        assert inc.split('"')[1] in ("../../include/tld_hip.h", "tld_guidance_shape.h", "tld_sampler_rows.h"), inc
    assert "hip/hip_runtime" not in hdr

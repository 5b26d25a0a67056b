"""The self-attention backward (csrc/tld_train_attn.hip) through tld_debug_attention_bwd: every instantiation of attn_bwd_kernel<NW, MODE, TG = float,
MASKED> that the dispatch can select, and every product grid, class by class against float64.

attn_bwd_block_waves and attn_bwd_dispatch are restated in tests/train_plan_ref.py (block_waves, dispatch; held against the C++ on the CPU by
tests/test_train_plan_host.py); CPU tests here hold the restatement against the
padded-work figures of the kernel file's header comment and the case table against everything the dispatch can select for N a multiple of 16 up
to 4096.  Each GPU case fills the output with NaN (every element must be written), keeps sentinels behind row B N and statistic 2 B H N, and
compares dq, dk and dv separately with the exact float64 backward (train_stage_refs.attn_bwd) of the same bf16-exact operands, over the whole
tensor and every member of every class: each (sample, head), the rows of the full blocks, of the last partial block, its final 16 rows when
N % 32 == 16, the first 32 rows, and the rows of each owning wave ((row % BT) // 32).  The bound of a member is the rule of
tests/test_gpu_forward_stages.py for its MODELLED transitions: MODEL_FACTOR x the relative rms of train_stage_refs.attn_bwd_model -- the same
float64 backward with the roundings the kernel documents -- against the exact result over the same member.

Input families: 1 random (q x 1.5, g = 0.1 randn) at every case; and at every masked instantiation and one exact one per mode: 2 gradient
confined to the last query block, to its final 16 rows, and to the first block (dq bitwise zero elsewhere); 3 keys of the tail aligned with
every query, P above 0.9 in the partial tile; 4 the forward test's rising scores; 5 every score q.k / 8 in log2 units inside -300 ... -150,
and mirrored inside 150 ... 300.  With TLD_ATTN_BWD_CLASS_RECORD=<file> every case appends yardstick / measured per class for dq | dk | dv,
and the last test the worst class per tensor (profiles/r11_attn_bwd_classes.txt).

The training step runs this same TG = float instantiation (tld_train.hip passes its fp32 residual gradient; the bf16-gradient overload of
launch_attention_bwd has no caller), so tests/test_gpu_train_stages.py compares the engine's dqkv with the fp32-gradient form of the model.

Found by family 5, confirmed on an MI355X with the parent build: in the masked two-kernel dQ kernel the second sweep applied no key mask, a
key past N got P = 2^-Lq = +inf once every real score of the row lay below -128 log2 units, and inf x 0 in the dQ product gave NaN -- every dq
value at N = 272, 336, 496 and 816 (the 5-, 6-, 8- and 4-wave masked pairs), dk and dv and the mirrored all-positive case unaffected, the
single-workgroup form (which masks before its one softmax) unaffected.  Fixed in the kernel: mask_keys before P in the last key block of
sweep 2.  tools/attn_bwd_ab_check.py dumps family 1 of every case for a bitwise comparison of two builds (TLD_LIB): parent and fixed build,
37 cases, 22 560 768 bf16 values, bitwise identical.

On the fixed build all 137 GPU tests pass (5.6 s run alone); over every case and class the worst measured / yardstick is 1.01 (dq), 1.10 (dk),
1.03 (dv): measured = yardstick, as the forward file finds for its MODELLED stages.

The checks bite.  Three one-line mutations, one library each (TLD_LIB), each run once on an MI355X: this file (137 GPU tests), then the older
test_attention_backward_vs_autograd / test_attention_backward_any_token_count_vs_autograd (12 tests, "old"):
  1 the masked ATTN_DKV kernel, kval with <= instead of <: 39 fail here -- every two-kernel masked case of every family: a dk / dv row written at
      token N (the sentinel behind row B N, or row 0 of the next sample, which also breaks run-to-run identity).  Old: 2 fail (400, 784, the sentinel).
  2 mask_keys, lim 4 lower for hi = 1 (the other direction changes nothing: N is a multiple of 16 and the rows come in runs of 4 per 8): 103 fail
      here -- every masked case, fused and two-kernel; random operands at N = 400: dq 1.1e-1 on the full blocks against a bound of 6.2e-3.
      Old: 4 fail (16, 144, 400, 784).
  3 stage_g, delta of the last row of a partial block taken from the row before: 99 fail here -- every masked case; random operands at N = 400:
      dq of the final 16 rows 9.4e-2 against 7.3e-3, dk over the whole tensor 1.1e-2 against 6.0e-3.  Old: 2 fail (16, 144: the single-workgroup
      form); 400, 784 and 3136 pass -- dk moves by 1.1e-2 of a 2e-2 bound, the one wrong dq row does not show in a whole-tensor figure.
"""
import ctypes as C
import math
import os

import pytest
import torch

import train_stage_refs as R
from test_gpu_forward_stages import MODEL_FACTOR, ROUND_C

gpu = pytest.mark.gpu
LOG2E = 1.44269504088896340736


# ---- the dispatch, restated: tests/train_plan_ref.py (held against csrc/tld_train_plan.h on the CPU by tests/test_train_plan_host.py) -----------------
from train_plan_ref import block_waves, dispatch  # noqa: E402,F401


def padded_work(n):
    bt = 32 * dispatch(n)[1]
    return (-(-n // bt) * bt / n) ** 2


def _smallest_two_kernel():
    first = {}
    for n in range(272, 4097, 16):
        first.setdefault(dispatch(n), n)
    return first


GRIDS = [(4 * i) ** 2 for i in range(1, 17)]                                         # every grid the trainer accepts
SINGLE = [32 * nw for nw in range(1, 9)] + [32 * nw - 16 for nw in range(1, 9)]      # the single-workgroup form, exact and masked
TWO = sorted(_smallest_two_kernel().values())                                        # the smallest N of every two-kernel instantiation
RANDOM_NS = sorted(set(GRIDS + SINGLE + TWO))
# families 2 .. 5: every masked instantiation at its smallest N, and one exact instantiation per mode (3 waves: odd; 6 waves, three blocks)
FAMILY_NS = sorted(n for n in SINGLE + TWO if dispatch(n)[2]) + [96, 576]


def _bh(n):
    return (3, 2) if n <= 1024 else (1, 3)          # a (sample, head) pair count that is not a multiple of 8 at the large ones


def test_dispatch_restatement_matches_the_padded_work_figures():
    want = {16: 4.0, 144: 1.23, 400: 1.44, 784: 1.04, 1296: 1.08, 1936: 1.12, 2704: 1.01, 3600: 1.03}
    for n, w in want.items():
        assert abs(padded_work(n) - w) < 0.005, (n, padded_work(n), w)
    for n in [576, 1600, 3136] + list(range(256, 4097, 256)):
        assert padded_work(n) == 1.0 and not dispatch(n)[2], n
    assert dispatch(1296) == ("two", 6, True) and dispatch(3600) == ("two", 6, True) and dispatch(1936) == ("two", 8, True)
    assert dispatch(784) == ("two", 5, True) and dispatch(1600) == ("two", 5, False) and dispatch(3136) == ("two", 7, False)
    assert all(dispatch(n)[1:] != (7, True) for n in range(272, 4097, 16))          # the masked 7-wave pair is never selected
    small = {k[1:]: n for k, n in _smallest_two_kernel().items()}
    # the smallest N of each two-kernel pair (272 = 8.5 x 32 already takes the 5-wave masked pair at two blocks, 448 = 2 x 224 the 7-wave one)
    assert small == {(4, True): 816, (4, False): 1408, (5, True): 272, (5, False): 320, (6, True): 336, (6, False): 384, (7, False): 448,
                     (8, True): 496, (8, False): 512}, small
    assert all(n % 32 == 16 for k, n in small.items() if k[1])                       # each masked one has a half-outside 32 x 32 tile
    assert 336 % 32 == 16


def test_case_table_covers_the_dispatch_and_every_product_grid():
    every = {dispatch(n) for n in range(16, 4097, 16)}
    assert len(every) == 16 + 9
    assert {dispatch(n) for n in RANDOM_NS} == every
    assert set(GRIDS) <= set(RANDOM_NS) and len(GRIDS) == 16 and GRIDS[-1] == 4096
    masked = {k for k in every if k[2]}
    assert {dispatch(n) for n in FAMILY_NS if dispatch(n)[2]} == masked
    assert {dispatch(n)[0] for n in FAMILY_NS if not dispatch(n)[2]} == {"fused", "two"}


# ---- inputs (host, bf16-exact operands) ---------------------------------------------------------------------------------------------------------
def _bf(t):
    return t.bfloat16().float()


def inputs(family, N, variant=0, bh=None):
    """(q, k, v, g) fp32 host tensors [B, N, d]; q, k, v bf16-exact.  bh: another (samples, heads) than this file's (the forward's grid tests)."""
    B, H = bh or _bh(N)
    d = 64 * H
    gen = torch.Generator().manual_seed(1000 * family + N + 7 * variant)
    rn = lambda *s: torch.randn(*s, generator=gen)
    bt = 32 * dispatch(N)[1]
    last0 = (N - 1) // bt * bt                                  # first row of the last query block
    q, k, v, g = rn(B, N, d) * 1.5, rn(B, N, d), rn(B, N, d), rn(B, N, d) * 0.1
    if family == 2:                                             # variant 0: g on the last block, 1: on its final 16 rows, 2: on the first block
        keep = torch.zeros(N, dtype=torch.bool)
        keep[(last0, N - 16, 0)[variant]:(N, N, min(bt, N))[variant]] = True
        g = g * keep.view(1, N, 1)
    elif family == 3:                                           # every query and the tail keys along one direction, the last key strongest
        T = 16 if N % 32 == 16 else 32
        q = 1.0 + 0.25 * rn(B, N, d)
        k = 0.25 * rn(B, N, d)
        k[:, N - T:] += torch.cat([torch.linspace(0.5, 1.25, T - 1), torch.tensor([2.0])]).view(1, T, 1)
    elif family == 4:                                           # tests/test_gpu_attention.py: all-positive queries, keys growing with their index
        q = rn(B, N, d).abs()
        k = torch.rand(B, N, d, generator=gen) * torch.linspace(0.05, 6.0, N).view(1, N, 1)
    elif family == 5:                                           # q = a u + noise, k = -+ a u + noise, |u| = 1: q.k = -+ a^2 + ..., a^2 / 8 log2(e) = 225
        a = math.sqrt(225.0 / (0.125 * LOG2E)) / 8.0
        q = a + 0.5 * rn(B, N, d)
        k = (a if variant else -a) + 0.5 * rn(B, N, d)
    return _bf(q), _bf(k), _bf(v), g


def log2_scores(q, k, H):
    B, N, d = q.shape
    sp = lambda t: t.double().view(B, N, H, 64).transpose(1, 2)
    return sp(q) @ sp(k).transpose(-1, -2) * (0.125 * LOG2E)


@pytest.mark.parametrize("N", [144, 400])
@pytest.mark.parametrize("variant", [0, 1])
def test_strongly_signed_scores_have_an_ordinary_float64_gradient(N, variant):
    """Family 5 on the CPU: every score lies in -300 ... -150 (mirrored: 150 ... 300) log2 units, the softmax is shift-invariant, and the
    float64 gradient is finite and non-trivial; so is the rounding model's."""
    q, k, v, g = inputs(5, N, variant)
    H = _bh(N)[1]
    s = log2_scores(q, k, H)
    lo, hi = float(s.min()), float(s.max())
    assert (150 < lo and hi < 300) if variant else (-300 < lo and hi < -150), (lo, hi)
    qd, kd, vd, gd = (t.double() for t in (q, k, v, g))
    exact = R.attn_bwd(qd, kd, vd, gd, H)
    p = torch.softmax(s / LOG2E, dim=-1)
    assert 0.02 < float(p.max(-1).values.mean()) < 0.9          # neither uniform nor one-hot
    model = R.attn_bwd_model(qd, kd, vd, R.bf16_round(R.attn_fwd(qd, kd, vd, H)), gd, H, False)
    for a, m in zip(exact, model):
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 1e-4
        # (dq and dk: the rows of dS sum to zero and K, Q carry the large common component a u, so the bf16 rounding of dS no longer cancels
        # against it -- the model shows some 4e-2 there, where random operands give 3e-3)
        assert bool(torch.isfinite(m).all()) and float((m - a).norm() / a.norm()) < 2.0 ** -3


# ---- one launch ----------------------------------------------------------------------------------------------------------------------------------
SENT = 1024.0            # exact in bf16 and fp32
PAD = 256                # the widest block


def launch(q, k, v, o, g, H):
    """tld_debug_attention_bwd on device copies of the host operands (o bf16 [B, N, d]): the raw bf16 output rows [B N, 3 d]; checks the sentinels."""
    from test_gpu_parity import _dev
    from transformer_latent_diffusion_amd import _lib
    B, N, d = q.shape
    dev = _dev()
    qk = torch.cat([q, k], dim=-1).bfloat16().to(dev).contiguous()
    vt = v.view(B, N, H, 64).permute(0, 2, 3, 1).contiguous().bfloat16().to(dev)
    ob, gd = o.to(dev).contiguous(), g.to(dev).contiguous()
    assert ob.dtype == torch.bfloat16 and gd.dtype == torch.float32
    out = torch.full((B * N + PAD, 3 * d), SENT, dtype=torch.bfloat16, device=dev)
    out[:B * N] = float("nan")
    scratch = torch.full((2 * B * H * N + 2 * PAD,), SENT, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().tld_debug_attention_bwd(C.c_void_p(qk.data_ptr()), C.c_void_p(vt.data_ptr()), C.c_void_p(ob.data_ptr()), C.c_void_p(gd.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(scratch.data_ptr()), B, N, H,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)), "attention_bwd")
    torch.cuda.synchronize()
    assert bool((out[B * N:] == SENT).all()), f"N={N}: {int((out[B * N:] != SENT).sum())} values written past row B N"
    assert bool((scratch[2 * B * H * N:] == SENT).all()), f"N={N}: statistics written past 2 B H N"
    return out[:B * N].clone()


def references(q, k, v, g, H):
    """float64 on the device, one (sample, head) at a time: (o as bf16 [B, N, d], exact (dq, dk, dv), model (dq, dk, dv))."""
    from test_gpu_parity import _dev
    dev = _dev()
    B, N, d = q.shape
    qd, kd, vd, gd = (t.to(dev).double() for t in (q, k, v, g))
    o = torch.empty(B, N, d, dtype=torch.bfloat16, device=dev)
    exact, model = torch.empty(3, B, N, d, dtype=torch.float64, device=dev), torch.empty(3, B, N, d, dtype=torch.float64, device=dev)
    for b in range(B):
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            one = [t[b:b + 1, :, c] for t in (qd, kd, vd, gd)]
            ob = R.attn_fwd(*one[:3], 1).float().bfloat16()
            o[b:b + 1, :, c] = ob
            for j, t in enumerate(R.attn_bwd(*one, 1)):
                exact[j, b, :, c] = t[0]
            for j, t in enumerate(R.attn_bwd_model(*one[:3], ob.double(), one[3], 1, False)):
                model[j, b, :, c] = t[0]
    return o, exact, model


# ---- classes and the comparison ----------------------------------------------------------------------------------------------------------------
def classes(got, ref, H, nw):
    """Relative rms of got against ref ([B, N, 64 H]) over every member of every class: {class: tensor over its members}.  The rule of
    tests/test_gpu_forward_stages.py: a member whose reference is (numerically) zero is held to the whole tensor's size."""
    B, N, _ = ref.shape
    bt = 32 * nw
    e2, r2 = ((got - ref) ** 2).view(B, N, H, 64).sum(-1), (ref ** 2).view(B, N, H, 64).sum(-1)          # [B, N, H]
    whole = float(r2.sum())
    out = {}

    def add(tag, es, rs):
        es, rs = es.reshape(-1), rs.reshape(-1)
        ok = rs > 1e-6 * whole / max(rs.numel(), 1)
        out[tag] = torch.where(ok, es / rs.clamp_min(1e-300), es / (whole / max(rs.numel(), 1))).sqrt()
    add("whole", e2.sum(), r2.sum())
    add("(sample, head)", e2.sum(1), r2.sum(1))
    full = N // bt * bt
    if full:
        add("full blocks", e2[:, :full].sum(), r2[:, :full].sum())
    if N % bt:
        add("last partial block", e2[:, full:].sum(), r2[:, full:].sum())
    if N % 32 == 16:
        add("final 16 rows", e2[:, N - 16:].sum(), r2[:, N - 16:].sum())
    add("first 32 rows", e2[:, :32].sum(), r2[:, :32].sum())
    wave = (torch.arange(N, device=ref.device) % bt) // 32
    ws = [w for w in range(nw) if bool((wave == w).any())]
    add("owning wave", torch.stack([e2[:, wave == w].sum() for w in ws]), torch.stack([r2[:, wave == w].sum() for w in ws]))
    return out


_WORST = {}              # tensor name -> (measured / yardstick, measured, yardstick, case, class): the summary of the record


def _record(line):
    path = os.environ.get("TLD_ATTN_BWD_CLASS_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def compare(case, got, exact, model, H, nw, K):
    """got [B, N, 3 d] float64 against exact / model [3, B, N, d]: the failures as text; prints and records every class."""
    B, N, _ = exact.shape[1:]
    d = 64 * H
    fail = []
    for j, name in enumerate(("dq", "dk", "dv")):
        g_ = got.view(B, N, 3, d)[:, :, j]
        bad = int((~torch.isfinite(g_)).sum())
        if bad:
            fail.append(f"{case} {name}: {bad} of {g_.numel()} values are NaN / Inf")
            _record(f"{case:44s} {name}: {bad} of {g_.numel()} values are NaN / Inf")
            continue
        yard = classes(model[j], exact[j], H, nw)
        if float(yard["whole"].max()) < 2.0 ** -11:          # the model says nothing: one rounding of the exact result (ROUND)
            bound = 2.0 ** -8 * exact[j].abs() + ROUND_C * math.sqrt(max(K, 64) / 64) * exact[j].abs().max()
            val = float(((g_ - exact[j]).abs() / bound).max())
            print(f"{case} {name}: model error near zero, ROUND {val:.3e} (bound 1)")
            if not val <= 1.0:
                fail.append(f"{case} {name} [round]: {val:.3e} > 1")
            continue
        meas = classes(g_, exact[j], H, nw)
        cells = []
        for tag in yard:
            i = int((meas[tag] / yard[tag].clamp_min(1e-300)).argmax())
            y, m = float(yard[tag][i]), float(meas[tag][i])
            cells.append(f"{tag} {y:.2e} / {m:.2e}")
            if not m <= MODEL_FACTOR * y:
                fail.append(f"{case} {name} ({tag}, member {i}): measured {m:.3e} > {MODEL_FACTOR} x yardstick {y:.3e}")
            if y > 0 and (name not in _WORST or m / y > _WORST[name][0]):
                _WORST[name] = (m / y, m, y, case, tag)
        line = f"{case:44s} {name}: yardstick / measured  " + "  ".join(cells)
        print(line)
        _record(line)
    return fail


def run_case(family, N, variant=0):
    B, H = _bh(N)
    mode, nw, masked = dispatch(N)
    q, k, v, g = inputs(family, N, variant)
    o, exact, model = references(q, k, v, g, H)
    assert bool(torch.isfinite(exact).all()) and float(exact.abs().max()) > 0
    raw = launch(q, k, v, o, g, H)
    case = f"family {family}.{variant} N={N} {mode} {nw}{' masked' if masked else ''} B={B} H={H}"
    return raw, compare(case, raw.double(), exact, model, H, nw, N), (q, k, v, o, g, exact)


# ---- GPU tests ---------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("N", RANDOM_NS)
def test_random_operands_every_instantiation_and_grid(N):
    _, fail, _ = run_case(1, N)
    assert not fail, "\n".join(fail)


@gpu
@pytest.mark.parametrize("N", FAMILY_NS)
@pytest.mark.parametrize("variant", [0, 1, 2])
def test_gradient_confined_to_one_block(N, variant):
    """g only on the last query block / its final 16 rows / the first block: dk and dv come through that block alone, dq is bitwise zero elsewhere."""
    raw, fail, (q, k, v, o, g, exact) = run_case(2, N, variant)
    B, H = _bh(N)
    d = 64 * H
    zero_rows = (g.view(B, N, d).abs().sum(-1) == 0).view(-1).to(raw.device)
    dq_bits = raw.view(torch.int16)[:, :d]
    assert int(zero_rows.sum()) > 0 or N <= 32 * dispatch(N)[1]
    assert not bool(dq_bits[zero_rows].any()), f"N={N}: dq of {int(dq_bits[zero_rows].any(-1).sum())} rows without a gradient is not bitwise zero"
    assert not fail, "\n".join(fail)


@gpu
@pytest.mark.parametrize("N", FAMILY_NS)
def test_probability_peaked_onto_the_tail_keys(N):
    q, k, v, g = inputs(3, N)
    p = torch.softmax(log2_scores(q, k, _bh(N)[1]) / LOG2E, dim=-1)
    T = 16 if N % 32 == 16 else 32
    assert float(p.max()) > 0.9 and float(p[..., N - T:].sum(-1).min()) > 0.99          # nearly all mass in the last (partial) tile
    _, fail, _ = run_case(3, N)
    assert not fail, "\n".join(fail)


@gpu
@pytest.mark.parametrize("N", FAMILY_NS)
def test_rising_scores(N):
    _, fail, _ = run_case(4, N)
    assert not fail, "\n".join(fail)


@gpu
@pytest.mark.parametrize("N", FAMILY_NS)
@pytest.mark.parametrize("variant", [0, 1])
def test_every_score_strongly_negative_or_positive(N, variant):
    """Every score below -150 (variant 1: above 150) log2 units: float64 is shift-invariant and finite; the kernel must be finite and inside the
    model bound (a key past N has score 0: 2^-Lq overflows there unless it is masked)."""
    q, k, v, g = inputs(5, N, variant)
    s = log2_scores(q, k, _bh(N)[1])
    lo, hi = float(s.min()), float(s.max())
    assert (150 < lo and hi < 300) if variant else (-300 < lo and hi < -150), (lo, hi)
    _, fail, _ = run_case(5, N, variant)
    assert not fail, "\n".join(fail)


@gpu
def test_masked_two_kernel_case_is_bitwise_reproducible():
    N = 400
    q, k, v, g = inputs(1, N)
    o, _, _ = references(q, k, v, g, _bh(N)[1])
    a, b = launch(q, k, v, o, g, _bh(N)[1]), launch(q, k, v, o, g, _bh(N)[1])
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


@gpu
def test_summary_of_measured_against_yardstick():
    """Last: the worst measured / yardstick per tensor over the cases this session ran (one case is run if none was), recorded."""
    if not _WORST:
        run_case(1, 400)
    for name, (ratio, m, y, case, tag) in sorted(_WORST.items()):
        line = (f"summary {name}: worst measured / yardstick {ratio:.2f} ({m:.2e} / {y:.2e}) in class '{tag}' of {case}; "
                f"measured {'~' if 0.8 <= ratio <= 1.25 else '!'}= yardstick there, bound {MODEL_FACTOR} x")
        print(line)
        _record(line)
        assert ratio <= MODEL_FACTOR


def dump_random(path):
    """tools/attn_bwd_ab_check.py: the raw bf16 output of family 1 at every case, concatenated, for a bitwise comparison of two builds."""
    import numpy as np
    rows = []
    for N in RANDOM_NS:
        q, k, v, g = inputs(1, N)
        H = _bh(N)[1]
        o, _, _ = references(q, k, v, g, H)
        rows.append(launch(q, k, v, o, g, H).view(torch.int16).cpu().numpy().reshape(-1))
    np.save(path, np.concatenate(rows))

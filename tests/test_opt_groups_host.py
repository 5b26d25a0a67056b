"""CPU: the host side of the grouped optimizer step -- the float64 statement (tests/opt_groups_ref.py) against
torch.optim.AdamW + LambdaLR + clip_grad_norm_ on float64 tensors, the planner (csrc/tld_opt_plan.h through tests/host/opt_plan_main.cpp, plain and
under AddressSanitizer + UBSan) against the restated cut, ``opt_groups`` on the real layouts, and the refusals of tld_opt_plan_create, which come
before any HIP call and so need no GPU."""
import ctypes as C
import inspect
import math
import os
import shutil
import subprocess
from dataclasses import asdict

import numpy as np
import pytest
import torch

import grad_guard_ref as R
import opt_groups_ref as G
from conftest import cfg_from_arr, load_golden
from transformer_latent_diffusion_amd import Denoiser, _lib, config_100m, opt_groups, param_layout

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, B1, B2, EPS, ALPHA = 3e-4, 0.9, 0.999, 1e-8, 0.999


def _tiny_cfg():
    return cfg_from_arr(load_golden("g15_train_step.npz")["cfg"])


LAYOUTS = {"g15_tiny": lambda: param_layout(_tiny_cfg()), "100m": lambda: param_layout(config_100m(32))}


def _close(a, b, tag):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (tag, float(np.abs(a - b).max()))


# ---- the float64 statement against torch --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clipped", [True, False])
def test_statement_equals_torch_adamw_lambdalr_and_clip_grad_norm_in_float64(clipped):
    """Four groups (neutral; scaled 0.1 with decay 0.05; decay 0 at scale 1; frozen = requires_grad False), seven tensors with ragged lengths, five
    steps of clip_grad_norm_ over the trainable tensors + AdamW.step() + LambdaLR.step() + update_ema, 1e-12 relative."""
    seg_numel = [37, 4, 130, 1, 64, 9, 255]
    seg_group = [0, 1, 2, 3, 1, 0, 3]
    groups = [(1.0, 0.01, False), (0.1, 0.05, False), (1.0, 0.0, False), (1.0, 0.01, True)]
    fn = opt_groups.warmup_cosine(2, 5, 0.1)
    table = [fn(j) for j in range(5)]
    n = sum(seg_numel)
    rng = np.random.default_rng(3)
    p0 = rng.standard_normal(n) * 0.05
    grads = [rng.standard_normal(n) * 1e-2 for _ in range(5)]
    offs = np.concatenate([[0], np.cumsum(seg_numel)])
    trainable = np.concatenate([np.arange(offs[i], offs[i + 1]) for i, q in enumerate(seg_group) if not groups[q][2]])
    norms = [float(np.linalg.norm(g[trainable])) for g in grads]
    max_norm = 0.5 * min(norms) if clipped else 2.0 * max(norms)
    ws = [torch.nn.Parameter(torch.from_numpy(p0[offs[i]:offs[i + 1]].copy()), requires_grad=not groups[q][2]) for i, q in enumerate(seg_group)]
    opt = torch.optim.AdamW([dict(params=[w for w, sq in zip(ws, seg_group) if sq == q], lr=LR * s, weight_decay=wd) for q, (s, wd, _) in enumerate(groups)],
                            lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, fn)
    e = torch.from_numpy(p0.copy())
    p, m, v, ema, st = p0.copy(), np.zeros(n), np.zeros(n), p0.copy(), R.fresh_state()
    for k, g in enumerate(grads):
        for i, w in enumerate(ws):
            w.grad = torch.from_numpy(g[offs[i]:offs[i + 1]].copy()) if w.requires_grad else None
        total = torch.nn.utils.clip_grad_norm_([w for w in ws if w.requires_grad], max_norm)
        opt.step()
        sched.step()
        flat = torch.cat([w.detach() for w in ws])
        e.mul_(ALPHA).add_(flat, alpha=1 - ALPHA)
        p, m, v, ema, st, seg_sq = G.grouped_step(p, g, m, v, ema, st, seg_numel, seg_group, groups, table, LR, B1, B2, EPS, ALPHA, 1.0, max_norm, False)
        _close(st[R.NORM], float(total), (k, "norm"))
        _close(np.sqrt(seg_sq), [np.linalg.norm(g[offs[i]:offs[i + 1]]) for i in range(len(seg_numel))], (k, "tensor norms"))
        assert (st[R.COEF] < 0.51) if clipped else (st[R.COEF] == 1.0)
        assert st[R.T] == k + 1 and st[G.FACTOR] == table[k]
        _close(p, flat.numpy(), (k, "params"))
        _close(ema, e.numpy(), (k, "ema"))
        for i, w in enumerate(ws):
            sl = slice(offs[i], offs[i + 1])
            if w.requires_grad:
                _close(m[sl], opt.state[w]["exp_avg"].numpy(), (k, i, "exp_avg"))
                _close(v[sl], opt.state[w]["exp_avg_sq"].numpy(), (k, i, "exp_avg_sq"))
            else:
                assert np.array_equal(p[sl], p0[sl]) and not m[sl].any() and not v[sl].any() and np.array_equal(ema[sl], p0[sl])
    assert np.abs(p - p0).max() > 1e-4


def test_statement_skip_keeps_the_factor_and_an_all_frozen_plan_only_counts():
    table = [0.25, 0.5, 1.0]
    st = G.finalize(R.fresh_state(), 4.0, 1.0, True, B1, B2, table)
    assert st[R.T] == 1 and st[G.FACTOR] == 0.25
    st2 = G.finalize(st, np.inf, 1.0, True, B1, B2, table)
    assert st2[R.LAST_SKIPPED] == 1 and st2[R.T] == 1 and st2[G.FACTOR] == 0.25
    st3 = G.finalize(st2, 4.0, 1.0, True, B1, B2, table)
    assert st3[R.T] == 2 and st3[G.FACTOR] == 0.5
    for _ in range(3):
        st3 = G.finalize(st3, 4.0, 1.0, True, B1, B2, table)
    assert st3[R.T] == 5 and st3[G.FACTOR] == 1.0                       # past the table the last entry holds
    assert G.finalize(R.fresh_state(), 4.0, 1.0, True, B1, B2, None)[G.FACTOR] == 1.0
    g = np.ones(10)
    p, m, v, ema, st, seg = G.grouped_step(g, g, 0 * g, 0 * g, g, R.fresh_state(), [4, 6], [0, 0], [(1.0, 0.1, True)], None, LR, B1, B2, EPS, ALPHA, 1.0, 1.0, True)
    assert st[R.NORM] == 0 and st[R.T] == 1 and np.array_equal(p, g) and not m.any() and list(seg) == [4.0, 6.0]


# ---- the planner ------------------------------------------------------------------------------------------------------------------------------
def _plan_cases():
    K = G.CHUNK
    cases = {"small": [1, 3, 4, 5, K - 1, K, K + 1], "ones": [1] * 9, "one_chunk": [K], "big": [2 ** 31 + 5], "big_between": [3, 2 ** 31 + 5, 1, K + 1],
             "mixed": [5, 2 * K, 2 * K + 1, 1, 3 * K - 1, 4]}
    for name, lay in LAYOUTS.items():
        cases[name] = [int(np.prod(s)) for _, s in lay().values()]
    return cases


def test_planner_cut_under_sanitizers_equals_the_restated_cut(tmp_path):
    """tests/host/opt_plan_main.cpp checks tiling, no chunk over two segments and exact ranges itself; its digests equal those of opt_groups_ref.cut.
    Built twice with the host compiler: plain, and with -fsanitize=address,undefined (run directly, nothing preloaded)."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    cases = _plan_cases()
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{k} {' '.join(map(str, v))}\n" for k, v in cases.items()))
    want = [f"{k} {' '.join(map(str, G.digest(v)))}" for k, v in cases.items()] + [f"chunk {G.CHUNK} 0 failures"]
    src = [os.path.join(REPO, "tests", "host", "opt_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / f"opt_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exe], check=True)
        r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-2000:])
        assert r.stdout.split("\n")[:-1] == want, (tag, r.stdout[-2000:])


def test_restated_cut_properties():
    K = G.CHUNK
    assert K % 4 == 0
    for name, seg in _plan_cases().items():
        first, length, sg, c0 = G.cut(seg)
        ends = np.cumsum(seg)
        assert first[0] == 0 and np.array_equal(first[1:], (first + length)[:-1]) and first[-1] + length[-1] == ends[-1], name
        assert length.min() >= 1 and length.max() <= K and np.all(first + length <= ends[sg]), name
        assert np.array_equal(np.bincount(sg, minlength=len(seg)), np.diff(c0)) and np.all(np.diff(sg) >= 0), name


# ---- opt_groups on the real layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_resolve_first_match_wins_default_is_group_0_and_no_decay_picks_vectors_and_the_position_table(name):
    lay = LAYOUTS[name]()
    keys = list(lay)
    nd = opt_groups.no_decay(lay)
    assert isinstance(nd, list) and len(nd) == 1 and nd[0]["weight_decay"] == 0.0
    want = [k for k, (_, s) in lay.items() if len(s) == 1 or k == "denoiser_trans_block.pos_embed.weight"]
    assert nd[0]["match"] == want and "denoiser_trans_block.pos_embed.weight" in want and "norm.weight" in want and "label_proj.weight" not in want
    specs = nd + [dict(match="label_proj.*", frozen=True), dict(match=["*decoder_blocks.*", "norm.*"], lr_scale=0.1, weight_decay=0.05)]
    seg_numel, seg_group, groups = opt_groups.resolve(lay, specs, 0.01)
    assert seg_numel == [int(np.prod(s)) for _, s in lay.values()] and len(seg_group) == len(keys)
    assert groups == [(1.0, 0.01, False), (1.0, 0.0, False), (1.0, 0.01, True), (0.1, 0.05, False)]
    by = dict(zip(keys, seg_group))
    assert by["label_proj.bias"] == 1 and by["label_proj.weight"] == 2                    # the bias met no_decay first
    assert by["norm.weight"] == 1                                                          # ... and so did the final norm, before the fourth spec
    assert by["denoiser_trans_block.decoder_blocks.0.mlp.mlp.0.weight"] == 3 and by["denoiser_trans_block.decoder_blocks.0.norm1.bias"] == 1
    assert by["fourier_feats.1.weight"] == 0 and by["denoiser_trans_block.pos_embed.weight"] == 1
    assert all((q == 1) == (k in want) for k, q in by.items())
    # no specs: one default group; an inherited and an explicit decay
    assert opt_groups.resolve(lay, None, 0.02)[1:] == ([0] * len(keys), [(1.0, 0.02, False)])
    assert opt_groups.resolve(lay, [dict(match="norm.*")], 0.02)[2] == [(1.0, 0.02, False), (1.0, 0.02, False)]
    with pytest.raises(ValueError, match="no_such_tensor"):
        opt_groups.resolve(lay, nd + [dict(match="no_such_tensor.*", frozen=True)], 0.0)
    with pytest.raises(ValueError):
        opt_groups.resolve(lay, [dict(match="norm.*", lr_scale=-1.0)], 0.0)
    with pytest.raises(ValueError):
        opt_groups.resolve(lay, [dict(match="norm.*", lr=1.0)], 0.0)


@pytest.mark.parametrize("fn", [opt_groups.warmup_cosine(3, 10, 0.1), opt_groups.warmup_constant(4), opt_groups.warmup_cosine(0, 5)])
def test_lr_table_follows_lambdalr(fn):
    """table[j] is the factor LambdaLR gives the optimizer for its step j + 1."""
    steps = 12
    table = opt_groups.lr_table(fn, steps)
    assert table.dtype == np.float32 and table.shape == (steps,)
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=1.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, fn)
    for j in range(steps):
        assert np.float32(opt.param_groups[0]["lr"]) == table[j], j          # the lr that step j + 1 runs at
        opt.step()
        sched.step()
    assert np.array_equal(opt_groups.lr_table([0.25, 1.0]), np.array([0.25, 1.0], dtype=np.float32))
    assert np.array_equal(opt_groups.lr_table([0.25, 1.0, 3.0], 2), np.array([0.25, 1.0], dtype=np.float32))
    for bad in ([], [1.0, -0.5], [float("nan")]):
        with pytest.raises(ValueError):
            opt_groups.lr_table(bad)
    with pytest.raises(ValueError):
        opt_groups.lr_table(fn)


def test_schedule_helpers_are_the_plain_formulas():
    f = opt_groups.warmup_cosine(2, 6, 0.1)
    assert [f(0), f(1)] == [0.5, 1.0] and f(5) == pytest.approx(0.1, abs=1e-15) and f(50) == pytest.approx(0.1, abs=1e-15)
    assert f(3) == 0.1 + 0.9 * 0.5 * (1.0 + math.cos(math.pi * 0.5))
    g = opt_groups.warmup_constant(4)
    assert [g(j) for j in range(6)] == [0.25, 0.5, 0.75, 1.0, 1.0, 1.0] and opt_groups.warmup_constant(0)(0) == 1.0


def test_torch_param_groups_load_into_adamw_on_a_cpu_model():
    cfg = _tiny_cfg()
    lay = param_layout(cfg)
    specs = opt_groups.no_decay(lay) + [dict(match="label_proj.*", frozen=True), dict(match="*decoder_blocks.*", lr_scale=0.1)]
    _, seg_group, groups = opt_groups.resolve(lay, specs, 0.01)
    tpg = opt_groups.torch_param_groups(seg_group, groups, LR, (B1, B2), EPS, lr_factor=0.5, scheduled=True)
    assert len(tpg) == len(groups) and sorted(i for g in tpg for i in g["params"]) == list(range(len(lay)))
    assert [g["lr"] for g in tpg] == [LR * s * 0.5 for s, _, _ in groups] and [g["initial_lr"] for g in tpg] == [LR * s for s, _, _ in groups]
    assert [g["weight_decay"] for g in tpg] == [wd for _, wd, _ in groups] and [g["frozen"] for g in tpg] == [f for _, _, f in groups]
    assert "initial_lr" not in opt_groups.torch_param_groups(seg_group, groups, LR)[0]
    params = list(Denoiser(**asdict(cfg)).parameters())
    assert len(params) == len(lay)
    opt = torch.optim.AdamW([dict(params=[params[i] for i in g["params"]]) for g in tpg], lr=1.0)
    opt.load_state_dict({"state": {}, "param_groups": tpg})
    for got, want in zip(opt.param_groups, tpg):
        assert got["lr"] == want["lr"] and got["weight_decay"] == want["weight_decay"] and tuple(got["betas"]) == (B1, B2) and got["eps"] == EPS
    opt.step()                                                                       # (no gradients: a no-op that must not trip over a key)


# ---- the C ABI without a GPU ------------------------------------------------------------------------------------------------------------------
def _create(seg_numel, seg_group, groups, factors, n_factors=None, out=True, n_seg=None, n_groups=None):
    L = _lib.lib()
    n = len(seg_numel) if seg_numel is not None else len(seg_group)
    numel = (C.c_int64 * max(n, 1))(*seg_numel) if seg_numel is not None else None
    group = (C.c_int32 * max(n, 1))(*seg_group) if seg_group is not None else None
    gs = (_lib.TldOptGroup * max(len(groups), 1))(*[_lib.TldOptGroup(*g) for g in groups]) if groups is not None else None
    tab = (C.c_float * max(len(factors), 1))(*factors) if factors is not None else None
    h = C.c_void_p()
    rc = L.tld_opt_plan_create(0, numel, group, n if n_seg is None else n_seg, gs, (len(groups) if groups is not None else 1) if n_groups is None else n_groups,
                               tab, (len(factors) if factors is not None else 0) if n_factors is None else n_factors, C.byref(h) if out else None)
    msg = L.tld_last_error()
    return rc, (msg or b"").decode(), h


def test_plan_create_refuses_bad_arguments_without_a_gpu():
    """TLD_ERR_INVALID with a text naming the offending index, before any HIP call."""
    ok_g = [(1.0, 0.0, 0, 0), (0.5, 0.1, 1, 0)]
    nan, inf = float("nan"), float("inf")
    cases = {
        "null seg_numel": (dict(seg_numel=None, seg_group=[0], groups=ok_g, factors=None, n_seg=1), "seg_numel is NULL"),
        "null seg_group": (dict(seg_numel=[4], seg_group=None, groups=ok_g, factors=None), "seg_group is NULL"),
        "null groups": (dict(seg_numel=[4], seg_group=[0], groups=None, factors=None), "groups is NULL"),
        "null out": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, out=False), "out is NULL"),
        "n_seg 0": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, n_seg=0), "n_seg 0"),
        "n_seg < 0": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, n_seg=-2), "n_seg -2"),
        "length 0": (dict(seg_numel=[4, 0, 3], seg_group=[0, 0, 0], groups=ok_g, factors=None), "segment 1: length 0"),
        "length < 0": (dict(seg_numel=[4, 2, -3], seg_group=[0, 0, 0], groups=ok_g, factors=None), "segment 2: length -3"),
        "n_groups 0": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, n_groups=0), "n_groups 0"),
        "n_groups 257": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, n_groups=257), "n_groups 257"),
        "group index 2": (dict(seg_numel=[4, 4], seg_group=[0, 2], groups=ok_g, factors=None), "segment 1: group 2"),
        "group index -1": (dict(seg_numel=[4, 4], seg_group=[-1, 0], groups=ok_g, factors=None), "segment 0: group -1"),
        "lr_scale < 0": (dict(seg_numel=[4], seg_group=[0], groups=[ok_g[0], (-0.5, 0.0, 0, 0)], factors=None), "group 1: lr_scale -0.5"),
        "lr_scale nan": (dict(seg_numel=[4], seg_group=[0], groups=[(nan, 0.0, 0, 0)], factors=None), "group 0: lr_scale nan"),
        "weight_decay inf": (dict(seg_numel=[4], seg_group=[0], groups=[ok_g[0], (1.0, inf, 0, 0)], factors=None), "group 1: weight_decay inf"),
        "weight_decay < 0": (dict(seg_numel=[4], seg_group=[0], groups=[(1.0, -1.0, 0, 0)], factors=None), "group 0: weight_decay -1"),
        "frozen 2": (dict(seg_numel=[4], seg_group=[0], groups=[ok_g[0], (1.0, 0.0, 2, 0)], factors=None), "group 1: frozen 2"),
        "n_factors < 0": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=[1.0], n_factors=-1), "n_factors -1"),
        "null table": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=None, n_factors=3), "lr_factors is NULL with n_factors 3"),
        "factor < 0": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=[1.0, 0.5, -0.25]), "lr factor 2: -0.25"),
        "factor nan": (dict(seg_numel=[4], seg_group=[0], groups=ok_g, factors=[nan, 0.5]), "lr factor 0: nan"),
        "total over 2^40": (dict(seg_numel=[2 ** 39, 2 ** 39, 1], seg_group=[0, 0, 0], groups=ok_g, factors=None), "segment 2: the total length passes 2^40"),
    }
    for tag, (kw, text) in cases.items():
        rc, msg, h = _create(**kw)
        assert rc == 1 and h.value is None, (tag, rc, msg)
        assert msg.startswith("opt plan: ") and text in msg, (tag, msg)


def test_step_calls_refuse_null_arguments_without_a_gpu_and_the_abi_has_the_entries():
    L = _lib.lib()
    for name in ("tld_opt_plan_create", "tld_opt_plan_destroy", "tld_opt_plan_numel", "tld_opt_plan_segment_sqsums", "tld_train_grad_guard_grouped",
                 "tld_train_adamw_ema_grouped"):
        assert name in _lib.ABI_SYMBOLS and hasattr(L, name), name
    assert C.sizeof(_lib.TldOptGroup) == 16
    assert L.tld_opt_plan_numel(None) == 0
    L.tld_opt_plan_destroy(None)
    buf = np.zeros(64, dtype=np.float64)
    g = C.c_void_p((buf.ctypes.data + 15) & ~15)
    assert L.tld_train_grad_guard_grouped(None, g, 8, 1.0, 1.0, 1, B1, B2, g, None) == 1 and b"grouped grad guard" in L.tld_last_error()
    assert L.tld_train_adamw_ema_grouped(None, g, g, g, g, None, 8, LR, B1, B2, EPS, ALPHA, 1.0, g, None) == 1 and b"grouped adamw" in L.tld_last_error()
    assert L.tld_opt_plan_segment_sqsums(None, None) == 1


def test_trainer_takes_the_group_keywords():
    from transformer_latent_diffusion_amd import Trainer
    sig = inspect.signature(Trainer.__init__).parameters
    assert sig["weight_decay"].default == 0.0 and sig["param_groups"].default is None and sig["lr_schedule"].default is None
    assert sig["schedule_steps"].default is None and isinstance(Trainer.tensor_grad_norms, property)

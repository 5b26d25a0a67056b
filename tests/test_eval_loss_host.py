"""CPU: the host side of the held-out loss -- the numpy statement of the accumulator by noise level against hand-made cases
and exact rational arithmetic, the batch / level plan of Trainer.eval_loss, and the refusals of the four C entries that precede any HIP call."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import eval_loss_ref as R
from transformer_latent_diffusion_amd import _lib
from transformer_latent_diffusion_amd.train import bucket_midpoints, eval_plan


# ---- the accumulator ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 10, 256])
def test_bucket_of_the_ends_and_of_every_bin_edge(n):
    assert R.bucket_index(0.0, n) == 0 and R.bucket_index(-0.0, n) == 0
    assert R.bucket_index(1.0, n) == n - 1                                    # floor(n) = n is clamped
    assert R.bucket_index(np.float32(1.0 - 2.0 ** -24), n) == n - 1           # the largest fp32 below 1: n - n 2^-24, floor n - 1
    for k in range(n + 1):
        lev = np.float32(k / n)                                               # the edge as fp32: above or below k / n by its rounding
        want = min(n - 1, int(Fraction(float(lev)) * n // 1))                 # exact rational arithmetic
        assert R.bucket_index(lev, n) == want, (k, n)
        assert want in (k - 1, k) or (k == n and want == n - 1)
    for bad in (-1e-30, -0.25, float("nan"), 1.5, np.float32(1.0 + 2.0 ** -23), float("inf"), float("-inf")):
        assert R.bucket_index(bad, n) == -1, bad


def test_known_edges_of_ten_buckets():
    """float32(0.1) = 0.100000001490116 and float32(0.3) = 0.300000011920929 lie above their edges, float32(0.7) = 0.699999988079071 and
    float32(0.9) = 0.899999976158142 below; k / 256 is exact."""
    assert [R.bucket_index(np.float32(x), 10) for x in (0.1, 0.3, 0.7, 0.9, 0.5)] == [1, 3, 6, 8, 5]
    assert [R.bucket_index(np.float32(k / 256), 256) for k in (0, 1, 17, 255, 256)] == [0, 1, 17, 255, 255]
    assert [R.bucket_index(x, 1) for x in (0.0, 0.5, 1.0)] == [0, 0, 0]


def test_accumulator_on_a_hand_made_batch():
    n = 4
    lev = np.array([0.0, 0.24, 0.25, 0.99, 1.0, -0.5, np.nan, 1.5, 0.5], dtype=np.float32)
    loss = np.array([1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0, 0.5])
    st = R.accumulate(R.fresh_state(n), loss, lev, n)
    assert st[:n].tolist() == [3.0, 4.0, 0.5, 24.0]
    assert st[n:2 * n].tolist() == [2.0, 1.0, 1.0, 2.0]
    assert st[2 * n] == 31.5 and st[2 * n + 1] == 3.0
    st2 = R.accumulate(st, loss, lev, n)                                      # a second call adds to the first
    assert np.array_equal(st2, 2 * st)
    total, per, cnt, rej = R.readout(st, n)
    assert total == 31.5 / 6 and per.tolist() == [1.5, 4.0, 0.5, 12.0] and rej == 3.0
    _, per0, _, _ = R.readout(R.accumulate(R.fresh_state(n), [1.0], np.float32([0.1]), n), n)
    assert per0[0] == 1.0 and np.isnan(per0[1:]).all()                        # NaN where a count is 0


def test_the_sum_is_the_serial_one():
    """1 + 2^-53 + 2^-53 in order is 1 (each addend is half an ulp: round to even); pairwise it would be 1 + 2^-52."""
    st = R.accumulate(R.fresh_state(1), [1.0, 2.0 ** -53, 2.0 ** -53], np.float32([0.5, 0.5, 0.5]), 1)
    assert st[0] == 1.0 and st[2] == 1.0 and st[1] == 3.0


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_a_nonfinite_loss_poisons_only_its_bucket_and_the_total(bad):
    n = 10
    lev = np.float32([0.05, 0.15, 0.25, 0.35])
    st = R.accumulate(R.fresh_state(n), [1.0, bad, 3.0, 4.0], lev, n)
    assert st[0] == 1.0 and st[2] == 3.0 and st[3] == 4.0 and not np.isfinite(st[1]) and not np.isfinite(st[2 * n])
    assert np.isfinite(st[n:2 * n]).all() and st[n:2 * n].sum() == 4.0 and st[2 * n + 1] == 0.0
    assert np.isfinite(np.delete(st, [1, 2 * n])).all()
    # a rejected sample's loss is never read into the sums
    st = R.accumulate(R.fresh_state(n), [1.0, bad], np.float32([0.05, 1.5]), n)
    assert np.isfinite(st).all() and st[2 * n] == 1.0 and st[2 * n + 1] == 1.0


def test_edge_levels_cover_what_the_device_tests_need():
    for n in (1, 10, 256):
        lev = R.edge_levels(n)
        idx = [R.bucket_index(x, n) for x in lev]
        assert idx.count(-1) == 3 and {0, n - 1} <= set(idx) and all(-1 <= k < n for k in idx) and len(idx) == n + 7


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,B", [(16, 4), (10, 4), (1, 4), (7, 7), (9, 2), (13, 128)])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_eval_plan_covers_every_position_once_and_assigns_levels_by_global_position(n, B, world):
    levels = bucket_midpoints(3)
    assert levels.tolist() == [0.5 / 3, 1.5 / 3, 2.5 / 3]
    seen = np.zeros(n, dtype=int)
    batches = []
    for rank in range(world):
        for j, start, stop, lv in eval_plan(n, B, world, rank, levels):
            assert j % world == rank and start == j * B and stop == min(n, start + B) and stop > start
            assert lv.dtype == np.float64 and np.array_equal(lv, levels[np.arange(start, stop) % 3])
            seen[start:stop] += 1
            batches.append(j)
    assert (seen == 1).all() and sorted(batches) == list(range((n + B - 1) // B))
    one = {j: lv for j, _, _, lv in eval_plan(n, B, 1, 0, levels)}              # the same batch carries the same levels at any world size
    for rank in range(world):
        for j, _, _, lv in eval_plan(n, B, world, rank, levels):
            assert np.array_equal(lv, one[j])


def test_eval_plan_ragged_tail_and_refusals():
    plan = eval_plan(10, 4, 1, 0, [0.0, 1.0])
    assert [(j, a, b) for j, a, b, _ in plan] == [(0, 0, 4), (1, 4, 8), (2, 8, 10)]
    assert plan[2][3].tolist() == [0.0, 1.0]
    assert eval_plan(10, 4, 3, 2, [0.5])[0][:3] == (2, 8, 10) and eval_plan(4, 4, 3, 1, [0.5]) == [] and eval_plan(0, 4, 1, 0, [0.5]) == []
    for bad in ([], [-0.1], [1.0 + 1e-12], [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            eval_plan(4, 4, 1, 0, bad)
    for kw in (dict(batch_size=0), dict(world=0), dict(rank=1), dict(rank=-1)):
        with pytest.raises(ValueError):
            eval_plan(**dict(dict(n=4, batch_size=4, world=1, rank=0, levels=[0.5]), **kw))


# ---- the C entries: part of the ABI, refusing before any HIP call -------------------------------------------------------------------------------
P = lambda v=0x1000: C.c_void_p(v) if v else None


def test_the_four_entries_are_part_of_the_abi():
    for s in ("tld_train_forward_loss", "tld_train_sample_loss", "tld_train_loss_buckets", "tld_train_prepare_batch_at"):
        assert s in _lib.ABI_SYMBOLS and hasattr(_lib.lib(), s), s


def test_loss_buckets_refuses_before_any_hip_call():
    L = _lib.lib()
    good = dict(sample=0x1000, level=0x1000, batch=4, n=10, state=0x1000)
    cases = [dict(sample=0), dict(level=0), dict(state=0), dict(state=0x1004), dict(sample=0x1004), dict(n=0), dict(n=-1), dict(n=257), dict(batch=0), dict(batch=-2)]
    for kw in cases:
        a = dict(good, **kw)
        assert L.tld_train_loss_buckets(P(a["sample"]), P(a["level"]), a["batch"], a["n"], P(a["state"]), None) == 1 and L.tld_last_error(), kw


def test_sample_loss_refuses_before_any_hip_call():
    L = _lib.lib()
    good = dict(rows=0x1000, batch=4, rps=16, elems=64, out=0x1000)
    cases = [dict(out=0), dict(out=0x1004), dict(batch=0), dict(batch=-1), dict(rps=0), dict(rps=-5), dict(elems=0), dict(elems=-1),
             dict(rows=0)]                                                     # no rows and no engine to take them from
    for kw in cases:
        a = dict(good, **kw)
        assert L.tld_train_sample_loss(None, P(a["rows"]), a["batch"], a["rps"], a["elems"], P(a["out"]), None) == 1 and L.tld_last_error(), kw


def test_forward_loss_refuses_a_null_engine():
    L = _lib.lib()
    assert L.tld_train_forward_loss(None, None, P(), P(), P(), P(), 4, P(), None, None, None) == 1 and L.tld_last_error()


def _prepare_at(src=None, idx=1, batch=4, a=1.0, b=2.5, p=0.0, outs=(1, 1, 1, 1), bad=1, level_in=0x2000, **src_kw):
    kw = dict(latents=0x1000, labels=0x1000, dequant_table=0x1000, rows=8, latent_dtype=_lib.DTYPE_U8, label_dtype=_lib.DTYPE_F16, latent_elems=64, text_emb=10,
              vae_scale=8.0)
    kw.update(src_kw)
    s = _lib.TldBatchSource(**kw)
    return _lib.lib().tld_train_prepare_batch_at(None, None if src == "null" else C.byref(s), P(idx and 0x1000), batch, 1, 2, 0, a, b, p,
                                                 *(P(o and 0x1000) for o in outs), None, None, None, P(bad and 0x1000), None, P(level_in))


@pytest.mark.parametrize("level_in", [0x2000, 0])
def test_prepare_batch_at_refuses_what_the_plain_entry_refuses(level_in):
    L = _lib.lib()
    cases = [dict(src="null"), dict(idx=0), dict(latents=None), dict(labels=None), dict(bad=0),
             dict(outs=(0, 1, 1, 1)), dict(outs=(1, 0, 1, 1)), dict(outs=(1, 1, 0, 1)), dict(outs=(1, 1, 1, 0)),
             dict(batch=0), dict(batch=-3), dict(rows=0), dict(latent_elems=0), dict(text_emb=0),
             dict(batch=(1 << 26) + 1), dict(batch=1 << 20, latent_elems=(1 << 14) + 1),
             dict(latent_dtype=_lib.DTYPE_BF16), dict(label_dtype=_lib.DTYPE_U8), dict(dequant_table=None),
             dict(latent_dtype=_lib.DTYPE_F16, vae_scale=0.0),
             dict(a=0.0), dict(a=float("nan")), dict(b=float("inf")), dict(p=-0.01), dict(p=1.01), dict(p=float("nan"))]
    for kw in cases:
        assert _prepare_at(level_in=level_in, **kw) == 1 and L.tld_last_error(), kw
    assert _prepare_at(level_in=0x2004) == 1 and b"aligned" in L.tld_last_error()

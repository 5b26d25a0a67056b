"""GPU: the held-out loss on the device -- tld_train_sample_loss, tld_train_loss_buckets, tld_train_prepare_batch_at and
tld_train_forward_loss through the C ABI, and Trainer.forward_loss / sample_loss / eval_loss / loss_buckets on the tiny g15 model at batch 4.

Bounds: a per-sample sum of at most 4096 positive terms in double is within rows * 2^-53 <= 4.6e-13 of the exact sum (held to 1e-12 against numpy's
float64 sum); the accumulator by noise level is the serial loop, so it is held bit for bit to its numpy statement (tests/eval_loss_ref.py); the mean
of the per-sample losses and the fp32 scalar loss differ by the fp32 roundings of loss_reduce_kernel -- each of 256 threads adds M / 256 positive
rows, the tree adds 8 levels, one product: (M / 256 + 10) * 2^-24 relative."""
import ctypes as C
import os
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import batch_prep_ref as BR  # noqa: F401  (the statement the plain entry is held to; the given-level entry is held to the plain one)
import eval_loss_ref as R
from test_gpu_batch_prep import CODES, LAT_DTYPES, _dataset, _source, _table
from test_gpu_grad_guard import _batches, _same_bits, _tiny
from test_gpu_train import _g15
from transformer_latent_diffusion_amd import EvalLoss, Trainer, TrainConfig, _lib
from transformer_latent_diffusion_amd.train import EVAL_SEED_XOR, bucket_midpoints, mix_noise

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev():
    return torch.device("cuda:0")


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64, 1: torch.uint8}[t.element_size()])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# ---- tld_train_sample_loss on synthetic rows -------------------------------------------------------------------------------------------------
def _sample_loss(rows, elems):
    """rows: host float32 [batch, R] -> host float64 [batch]"""
    dev = _dev()
    r = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    out = torch.full((r.shape[0],), -1.0, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tld_train_sample_loss(None, _p(r), r.shape[0], r.shape[1], elems, _p(out), _stream()), "tld_train_sample_loss")
    return out.cpu().numpy()


@pytest.mark.parametrize("batch", [1, 3, 128])
@pytest.mark.parametrize("rps", [1, 16, 63, 64, 65, 256, 4096])
def test_sample_loss_against_float64_sums(rps, batch):
    rng = np.random.default_rng(1000 * rps + batch)
    rows = (10.0 ** rng.uniform(-8.0, 4.0, (batch, rps))).astype(np.float32)
    elems = 3 * rps + 1
    ref = rows.astype(np.float64).sum(axis=1) / elems
    got, again = _sample_loss(rows, elems), _sample_loss(rows, elems)
    err = float((np.abs(got - ref) / ref).max())
    print(f"rows_per_sample {rps} batch {batch}: worst relative error {err:.2e} (bound 1e-12)")
    assert err <= 1e-12
    assert np.array_equal(got.view(np.int64), again.view(np.int64))                       # bitwise repeatable
    # a sample's value does not depend on its position, nor on the batch it sits in
    rolled = _sample_loss(np.roll(rows, 1, axis=0), elems)
    assert np.array_equal(np.roll(rolled, -1).view(np.int64), got.view(np.int64))
    alone = _sample_loss(rows[-1:], elems)
    assert alone.view(np.int64)[0] == got.view(np.int64)[-1]
    # one NaN row and one Inf row make exactly their samples non-finite
    for bad, where in ((np.nan, rps - 1), (np.inf, 0)):
        for b in sorted({0, batch - 1, batch // 2}):
            dirty = rows.copy()
            dirty[b, where] = bad
            out = _sample_loss(dirty, elems)
            assert not np.isfinite(out[b]) and (np.isnan(out[b]) if np.isnan(bad) else out[b] == np.inf)
            keep = np.arange(batch) != b
            assert np.array_equal(out[keep].view(np.int64), got[keep].view(np.int64))


# ---- tld_train_loss_buckets ----------------------------------------------------------------------------------------------------------------
def _buckets(state, loss, level, n):
    dev = _dev()
    l, v = torch.from_numpy(np.ascontiguousarray(loss, dtype=np.float64)).to(dev), torch.from_numpy(np.ascontiguousarray(level, dtype=np.float32)).to(dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tld_train_loss_buckets(_p(l), _p(v), l.numel(), n, _p(state), _stream()), "tld_train_loss_buckets")


def _level_pool(n, count, rng):
    e = R.edge_levels(n)
    pool = np.concatenate([e[:3], e[-3:], e[3:-3], rng.uniform(0.0, 1.0, max(0, count)).astype(np.float32)])
    return pool


@pytest.mark.parametrize("batch", [1, 4, 1000])
@pytest.mark.parametrize("n", [1, 10, 256])
def test_loss_buckets_equal_the_serial_loop_bit_for_bit_after_three_calls(n, batch):
    rng = np.random.default_rng(100 * n + batch)
    pool = _level_pool(n, 3 * batch, rng)
    if batch == 1000:
        assert pool.size >= 3 * batch and n + 7 <= batch                                  # every edge level is in the first call
    state = torch.zeros(2 * n + 2, dtype=torch.float64, device=_dev())
    ref = R.fresh_state(n)
    for call in range(3):
        lev = pool[call * batch:(call + 1) * batch]
        loss = 10.0 ** rng.uniform(-6.0, 2.0, batch)
        _buckets(state, loss, lev, n)
        ref = R.accumulate(ref, loss, lev, n)
    got = state.cpu().numpy()
    assert np.array_equal(got.view(np.int64), ref.view(np.int64)), (got, ref)
    assert got[n:2 * n].sum() + got[2 * n + 1] == 3 * batch


def test_loss_buckets_rejected_levels_and_nonfinite_losses():
    n = 10
    lev = np.array([0.05, -0.25, np.nan, 1.5, 0.15, 0.15, 0.95, 1.0], dtype=np.float32)
    loss = np.array([1.0, 2.0, 3.0, np.inf, np.nan, 5.0, np.inf, 7.0])
    state = torch.zeros(2 * n + 2, dtype=torch.float64, device=_dev())
    _buckets(state, loss, lev, n)
    got, ref = state.cpu().numpy(), R.accumulate(R.fresh_state(n), loss, lev, n)
    assert np.array_equal(got, ref, equal_nan=True)
    assert got[0] == 1.0 and np.isnan(got[1]) and got[9] == np.inf and np.isnan(got[2 * n]) and got[2 * n + 1] == 3.0
    assert got[n:2 * n].tolist() == [1, 2, 0, 0, 0, 0, 0, 0, 0, 2]
    assert np.isfinite(np.delete(got, [1, 9, 2 * n])).all()


# ---- tld_train_prepare_batch_at -----------------------------------------------------------------------------------------------------------
def _prep(lat, lab, idx, *, table=None, seed=1, step=0, replica=0, p=0.15, level_in="plain"):
    """level_in "plain": tld_train_prepare_batch; None: the _at entry with NULL; a device fp64 tensor: the given levels."""
    dev = lat.device
    B, E, T = idx.numel(), lat.shape[1], lab.shape[1]
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(x_noisy=f(B, E), noise_level=f(B), label=f(B, T), target=f(B, E), noise=f(B, E), noise_level64=torch.empty(B, dtype=torch.float64, device=dev),
               mask=torch.empty(B, dtype=torch.uint8, device=dev), bad=torch.zeros(1, dtype=torch.int32, device=dev))
    src = _lib.TldBatchSource(_p(lat), _p(lab), _p(table), lat.shape[0], CODES[lat.dtype], CODES[lab.dtype], E, T, 8.0)
    args = [None, C.byref(src), _p(idx), B, seed, step, replica, 1.0, 2.5, p] + [_p(out[k]) for k in ("x_noisy", "noise_level", "label", "target", "noise",
                                                                                                       "noise_level64", "mask", "bad")] + [_stream()]
    with torch.cuda.device(dev):
        if isinstance(level_in, str):
            _lib.check(_lib.lib().tld_train_prepare_batch(*args), "tld_train_prepare_batch")
        else:
            _lib.check(_lib.lib().tld_train_prepare_batch_at(*args, _p(level_in)), "tld_train_prepare_batch_at")
    return out


@pytest.mark.parametrize("E", [64, 27])
@pytest.mark.parametrize("lat_name", list(LAT_DTYPES))
def test_prepare_batch_at_given_levels(lat_name, E):
    """E = 64: the 16-byte path; E = 27: the element path, with Philox counters that straddle two samples."""
    dev = _dev()
    lat, lab = _source(9, E, 10, LAT_DTYPES[lat_name], torch.float16, seed=E)
    idx = torch.tensor([8, 0, 3, 3, 7]).to(dev)
    tab = _table().to(dev) if lat_name == "u8" else None
    kw = dict(table=tab, seed=0xABCDEF0123, step=(2 << 32) + 5, replica=1)
    lat, lab = lat.to(dev), lab.to(dev)
    plain = _prep(lat, lab, idx, **kw)
    null = _prep(lat, lab, idx, level_in=None, **kw)
    for k in plain:
        assert _same(plain[k], null[k]), k                                                # NULL is the plain entry
    levels = torch.tensor([0.0, 1.0, 0.5, 1e-300, 0.3], dtype=torch.float64)
    at = _prep(lat, lab, idx, level_in=levels.to(dev), **kw)
    for k in ("noise", "target", "label", "mask", "bad"):
        assert _same(plain[k], at[k]), k
    assert _same(at["noise_level64"].cpu(), levels) and _same(at["noise_level"].cpu(), levels.float())
    want = mix_noise(at["target"].cpu().view(5, E, 1, 1), levels, at["noise"].cpu().view(5, E, 1, 1)).view(5, E)
    assert _same(at["x_noisy"].cpu(), want)
    assert _same(at["x_noisy"][0], at["target"][0]) and _same(at["x_noisy"][1], at["noise"][1])      # levels 0 and 1
    assert not _same(at["x_noisy"], plain["x_noisy"])
    back = _prep(lat, lab, idx, level_in=plain["noise_level64"].clone(), **kw)            # the plain call's own draw, fed back
    for k in plain:
        assert _same(plain[k], back[k]), k


# ---- Trainer.forward_loss / sample_loss -----------------------------------------------------------------------------------------------------
def _loss_bound(tokens_total):
    return (tokens_total / 256 + 10) * 2.0 ** -24


@pytest.mark.parametrize("order", ["train_first", "loss_first"])
def test_forward_loss_is_the_training_forward_bit_for_bit_and_leaves_the_gradients(order):
    (batch,) = _batches(1)
    tr = _tiny()
    if order == "train_first":
        loss_t, pred_t = tr.forward_backward(*batch)
        loss_t, grads = loss_t.clone(), tr.grads.clone()
        loss, sample, pred = tr.forward_loss(*batch)
    else:
        loss, sample, pred = tr.forward_loss(*batch)
        assert float(tr.grads.abs().max()) == 0.0                                         # nothing has written them yet
        loss_t, pred_t = tr.forward_backward(*batch)
        grads = tr.grads.clone()
        tr.forward_loss(*batch)
    assert _same(loss, loss_t) and _same(pred, pred_t) and loss.data_ptr() != tr._loss.data_ptr()
    assert _same(tr.grads, grads) and float(grads.abs().max()) > 0                        # bit-unchanged by the call
    assert sample.dtype == torch.float64 and tuple(sample.shape) == (4,) and _same(tr.sample_loss(), sample)
    mean, l32 = float(sample.mean()), float(loss)
    rel = abs(mean - l32) / mean
    print(f"{order}: mean(sample_loss) {mean:.10g}, fp32 loss {l32:.10g}, relative {rel:.2e} (bound {_loss_bound(4 * 256):.2e})")
    assert rel <= _loss_bound(4 * 256)
    ref = ((pred.double() - batch[3].to(_dev()).double()) ** 2).mean(dim=(1, 2, 3))
    assert float(((sample - ref).abs() / ref).max()) <= 1e-5                              # fp32 squares in the rows; the double sum adds nothing to that
    assert tr.global_step == 1 and tr.step == 0


def test_sample_loss_after_a_debug_step_is_the_float64_sum_of_the_row_loss_stage_and_forward_loss_is_refused():
    (batch,) = _batches(1)
    tr = _tiny()
    with pytest.raises(RuntimeError, match="no forward"):
        tr.sample_loss()
    tr.set_debug(True)
    tr.forward_backward(*batch)
    got = tr.sample_loss().cpu().numpy()
    rows = tr.read_stage("row_loss").numpy().astype(np.float64).reshape(4, -1)
    ref = rows.sum(axis=1) / (4 * 32 * 32)
    assert rows.shape[1] == 256 and float((np.abs(got - ref) / ref).max()) <= 1e-12
    grads = tr.grads.clone()
    with pytest.raises(RuntimeError, match=r"status 4"):                                  # TLD_ERR_STATE: the stage hook is on
        tr.forward_loss(*batch)
    assert _same(tr.grads, grads)
    tr.set_debug(False)
    loss, sample, _ = tr.forward_loss(*batch)
    assert np.array_equal(sample.cpu().numpy().view(np.int64), got.view(np.int64))


def test_forward_loss_on_a_16_token_model():
    """image_size 8 at patch 2: 16 rows per sample, a quarter of a wave."""
    _, cfg, _ = _g15()
    cfg16 = replace(cfg, image_size=8)
    tr = Trainer(cfg16, TrainConfig(lr=3e-4, batch_size=4), device=_dev(), init_seed=4, max_batch=4, use_graph=False)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(3, 4, 8, 8, generator=g) * 0.8, torch.randn(3, 768, generator=g) * 0.5
    nl = torch.tensor([0.1, 0.5, 0.9])
    xn = mix_noise(x, nl, torch.randn(3, 4, 8, 8, generator=g))
    loss, sample, pred = tr.forward_loss(xn, nl, y, x)
    loss_t, pred_t = tr.forward_backward(xn, nl, y, x)
    assert _same(loss, loss_t) and _same(pred, pred_t) and _same(tr.sample_loss(), sample)
    ref = ((pred.double() - x.to(_dev()).double()) ** 2).mean(dim=(1, 2, 3))
    assert float(((sample - ref).abs() / ref).max()) <= 1e-5
    assert abs(float(sample.mean()) - float(loss)) <= _loss_bound(3 * 16) * float(sample.mean())


def test_forward_loss_on_the_ema_weights_equals_a_trainer_loaded_from_them():
    b0, b1, probe = _batches(3)
    a = _tiny()
    for batch in (b0, b1):
        a.forward_backward(*batch); a.optimizer_step()
    assert not torch.equal(a.ema, a.params)
    b = _tiny().load_state_dict(a.ema_state_dict())
    want = b.forward_loss(*probe)
    live = a.forward_loss(*probe, weights="model")
    for got in (a.forward_loss(*probe, weights="ema"), a.forward_loss(*probe, weights=a.ema.clone())):
        assert all(_same(x, y) for x, y in zip(got, want))
    assert not _same(live[0], want[0])
    assert all(_same(x, y) for x, y in zip(a.forward_loss(*probe), live))                 # and back on the bound parameters: the copies were rebuilt
    with pytest.raises(ValueError):
        a.forward_loss(*probe, weights="best")
    with pytest.raises(ValueError):
        a.forward_loss(*probe, weights=a.ema[:-1])


# ---- Trainer.eval_loss ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_an_evaluation_between_steps_changes_nothing_of_the_training(graph, accumulate):
    """A runs an eval_loss on the EMA weights before its last forward_backward (between two micro-batches when accumulating), B does not."""
    ds = _dataset()
    batches = _batches(3)
    a, b = _tiny(use_graph=graph), _tiny(use_graph=graph)
    losses = {id(a): [], id(b): []}
    for tr in (a, b):
        for k, batch in enumerate(batches):
            if tr is a and k == 2:
                acc_before = None if tr._acc is None else tr._acc.clone()
                step, gstep, n_acc = tr.step, tr.global_step, tr._acc_n
                res = tr.eval_loss(ds, torch.arange(16), batch_size=4)
                assert (tr.step, tr.global_step, tr._acc_n) == (step, gstep, n_acc)
                assert acc_before is None or _same(tr._acc, acc_before)
                assert float(res.bucket_count.sum()) == 16
            last = not (accumulate and k == 1)
            loss, _ = tr.forward_backward(*batch, last_micro_batch=last)
            losses[id(tr)].append(float(loss))
            if last:
                tr.optimizer_step()
    assert _same_bits(a, b) and losses[id(a)] == losses[id(b)] and a.global_step == b.global_step == 3 and a.step == b.step
    assert (a._graph is not None) == graph


def _eval_by_hand(tr, ds, rows, B, levels, key, n_buckets, weights="ema"):
    """The numpy statement fed with each batch's own sample_loss and levels."""
    dev = _dev()
    ref = R.fresh_state(n_buckets)
    lat, lab = ds.latents.view(len(ds), -1), ds.text_emb
    for j in range((len(rows) + B - 1) // B):
        pos = np.arange(j * B, min(len(rows), (j + 1) * B))
        lev = torch.from_numpy(np.asarray(levels, dtype=np.float64)[pos % len(levels)]).to(dev)
        out = _prep(lat, lab, torch.as_tensor(rows[pos]).to(dev), table=ds.table, seed=key, step=j, replica=0, p=0.0, level_in=lev)
        shape = (len(pos), 4, 32, 32)
        _, sample, _ = tr.forward_loss(out["x_noisy"].view(shape), out["noise_level"], out["label"], out["target"].view(shape), weights=weights)
        ref = R.accumulate(ref, sample.cpu().numpy(), out["noise_level"].cpu().numpy(), n_buckets)
    return ref


def test_eval_loss_over_16_rows_in_batches_of_4():
    ds = _dataset()
    tr = _tiny(data_seed=77)
    (batch,) = _batches(1)
    tr.forward_backward(*batch); tr.optimizer_step()                                      # EMA and live weights differ
    rows = np.arange(16)
    res = tr.eval_loss(ds, rows, batch_size=4)
    assert isinstance(res, EvalLoss) and res.state.is_cuda and res.state.dtype == torch.float64 and res.n_buckets == 10
    got = res.state.cpu().numpy()
    ref = _eval_by_hand(tr, ds, rows, 4, bucket_midpoints(10), 77 ^ EVAL_SEED_XOR, 10)
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    assert got[10:20].tolist() == [2, 2, 2, 2, 2, 2, 1, 1, 1, 1] and got[21] == 0        # position p at midpoint p % 10
    again = tr.eval_loss(ds, torch.arange(16, device=_dev()), batch_size=4)               # a device index vector, a second call
    assert _same(again.state, res.state)
    tr.global_step += 5                                                                   # the training-side counter is not part of the address
    assert _same(tr.eval_loss(ds, rows, batch_size=4).state, res.state)
    other = tr.eval_loss(ds, rows, batch_size=4, seed=123)
    assert not _same(other.state[:10], res.state[:10]) and _same(other.state[10:20], res.state[10:20])
    live = tr.eval_loss(ds, rows, batch_size=4, weights="model")
    assert not _same(live.state[:10], res.state[:10])
    # readouts
    loss, per, cnt, rej = R.readout(got, 10)
    d = res.cpu()
    assert d["loss"] == float(res.loss) == loss and np.array_equal(d["bucket_loss"], per) and np.array_equal(res.bucket_loss.cpu().numpy(), per)
    assert d["bucket_count"].tolist() == cnt.tolist() == res.bucket_count.cpu().tolist() and d["rejected"] == int(res.rejected) == 0
    assert np.isfinite(per).all() and (per > 0).all()
    assert tr.global_step == 6 and tr.step == 1


def test_eval_loss_with_given_levels_a_ragged_tail_and_empty_buckets():
    ds = _dataset(lat_dtype=torch.float16)
    tr = _tiny(data_seed=3)
    rows = np.array([5, 1, 1, 14, 0, 9, 2, 3, 8, 15])
    levels = [0.0, 1.0, 0.3]
    res = tr.eval_loss(ds, rows, noise_levels=levels, n_buckets=4, batch_size=4, seed=9)
    ref = _eval_by_hand(tr, ds, rows, 4, levels, 9, 4)
    got = res.state.cpu().numpy()
    assert np.array_equal(got.view(np.int64), ref.view(np.int64))
    assert got[4:8].tolist() == [4, 3, 0, 3] and np.isnan(res.cpu()["bucket_loss"][2]) and bool(torch.isnan(res.bucket_loss[2]))
    full = tr.eval_loss(ds, rows, noise_levels=levels, n_buckets=4, seed=9)               # batch_size = max_batch = 4
    assert _same(full.state, res.state)
    for bad in ([0.5, 1.5], [-0.1], [float("nan")], []):
        with pytest.raises(ValueError):
            tr.eval_loss(ds, rows, noise_levels=bad)
    with pytest.raises(ValueError):
        tr.eval_loss(ds, rows, batch_size=5)
    with pytest.raises(IndexError):
        tr.eval_loss(ds, [0, 16])


_RANK = r"""
import os, sys, numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
from transformer_latent_diffusion_amd import DenoiserConfig, DeviceLatentDataset, TrainConfig, Trainer
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
cfg = DenoiserConfig(image_size=32, n_channels=4)
tr = Trainer(cfg, TrainConfig(lr=3e-4), device=dev, init_seed=3, max_batch=4, data_seed=11)
g = torch.Generator().manual_seed(31)
ds = DeviceLatentDataset(torch.randint(0, 256, (16, 4, 32, 32), generator=g).to(torch.uint8), (torch.randn(16, 768, generator=g) * 0.5).half(), device=dev)
res = tr.eval_loss(ds, torch.arange(14), batch_size=4)
local = tr.eval_loss(ds, torch.arange(14), batch_size=4, reduce=False)
torch.cuda.synchronize()
torch.save(dict(state=res.state.cpu(), local=local.state.cpu()), {out!r} + f".{{w}}.{{r}}")
print("rank", r, "done")
"""


def test_two_ranks_split_the_batches_and_reduce_to_the_single_process_result(tmp_path):
    script = tmp_path / "rank.py"
    out = str(tmp_path / "state")
    script.write_text(_RANK.format(repo=REPO, out=out))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    for w in (2, 1):
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={w}", "--master-addr", "127.0.0.1",
                            "--master-port", "29583", str(script)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    a, b, one = (torch.load(out + s, weights_only=False) for s in (".2.0", ".2.1", ".1.0"))
    n = 10
    assert torch.equal(a["state"], b["state"]) and torch.equal(one["state"], one["local"])
    assert a["local"][n:2 * n].sum() == 8 and b["local"][n:2 * n].sum() == 6               # batches 0, 2 (4 + 4) and 1, 3 (4 + 2)
    assert torch.equal(a["local"] + b["local"], a["state"])
    assert torch.equal(a["state"][n:2 * n], one["state"][n:2 * n]) and a["state"][2 * n + 1] == one["state"][2 * n + 1] == 0
    sums = torch.cat([a["state"][:n], a["state"][2 * n:2 * n + 1]])
    want = torch.cat([one["state"][:n], one["state"][2 * n:2 * n + 1]])
    rel = float(((sums - want).abs() / want).max())
    print(f"two ranks against one process: worst relative difference of the sums {rel:.2e}")
    assert rel <= 1e-12


# ---- Trainer(loss_buckets=n) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True])
def test_loss_buckets_bookkeeping_changes_no_parameter_and_equals_the_statement(graph):
    batches = _batches(3)
    a, b = _tiny(loss_buckets=10, use_graph=graph), _tiny(use_graph=graph)
    assert b.train_loss_levels is None and isinstance(a.train_loss_levels, EvalLoss)
    with pytest.raises(RuntimeError):
        b.reset_loss_levels()
    ref = R.fresh_state(10)
    for k, batch in enumerate(batches):
        if k == 2:        # a short forward in between: the replayed step's batch is still the one sample_loss takes
            a.forward_loss(*(t[:2] for t in batch))
        for tr in (a, b):
            tr.forward_backward(*batch)
        ref = R.accumulate(ref, b.sample_loss().cpu().numpy(), batch[1].numpy(), 10)
        for tr in (a, b):
            tr.optimizer_step()
    assert _same_bits(a, b) and (a._graph is not None) == graph
    got = a.train_loss_levels.state.cpu().numpy()
    assert np.array_equal(got.view(np.int64), ref.view(np.int64)) and got[10:20].sum() == 12
    a.reset_loss_levels()
    assert float(a.train_loss_levels.state.abs().max()) == 0.0

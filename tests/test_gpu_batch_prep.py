"""GPU: the device batch preparation (tld_train_prepare_batch, csrc/tld_batch.hip) against its numpy statement
(tests/batch_prep_ref.py) -- bit for bit where the statement is exact (gather, dequantisation, label mask, the double mix), against float64 and
against the distributions where it is not (Box-Muller normals, the Beta draw) -- and through Trainer.prepare_batch / train_step_from."""
import ctypes as C

import numpy as np
import pytest
import torch

import batch_prep_ref as R
from test_gpu_grad_guard import _same_bits, _tiny
from transformer_latent_diffusion_amd import DeviceLatentDataset, _lib, dequantize_latents
from transformer_latent_diffusion_amd.train import mix_noise

pytestmark = pytest.mark.gpu

KS_ALPHA_001 = 1.95                      # the alpha = 0.001 critical value of sqrt(n) D_n
LAT_DTYPES = {"u8": torch.uint8, "f16": torch.float16, "f32": torch.float32}
LAB_DTYPES = {"f16": torch.float16, "f32": torch.float32}
CODES = {torch.uint8: _lib.DTYPE_U8, torch.float16: _lib.DTYPE_F16, torch.float32: _lib.DTYPE_F32}


def _dev():
    return torch.device("cuda:0")


def _table(clip_val=20, scale=8.0):
    return dequantize_latents(torch.arange(256), clip_val).float() / scale


def _prepare(lat, lab, idx, *, table=None, scale=8.0, seed=1, step=0, replica=0, a=1.0, b=2.5, p=0.15, debug=True, bad=None):
    """One call of the C entry without an engine on device tensors lat [rows, E], lab [rows, text], idx int64 [batch]."""
    dev = lat.device
    B, E, T = idx.numel(), lat.shape[1], lab.shape[1]
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(x_noisy=f(B, E), noise_level=f(B), label=f(B, T), target=f(B, E),
               noise=f(B, E) if debug else None, noise_level64=torch.empty(B, dtype=torch.float64, device=dev) if debug else None,
               mask=torch.empty(B, dtype=torch.uint8, device=dev) if debug else None,
               bad=bad if bad is not None else torch.zeros(1, dtype=torch.int32, device=dev))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    src = _lib.TldBatchSource(ptr(lat), ptr(lab), ptr(table), lat.shape[0], CODES[lat.dtype], CODES[lab.dtype], E, T, scale)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().tld_train_prepare_batch(None, C.byref(src), ptr(idx), B, seed, step, replica, a, b, p, ptr(out["x_noisy"]), ptr(out["noise_level"]),
                                                      ptr(out["label"]), ptr(out["target"]), ptr(out["noise"]), ptr(out["noise_level64"]), ptr(out["mask"]),
                                                      ptr(out["bad"]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_train_prepare_batch")
    return out


def _source(rows, E, T, lat_dtype, lab_dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    lat = torch.randint(0, 256, (rows, E), generator=g).to(torch.uint8) if lat_dtype == torch.uint8 else (torch.randn(rows, E, generator=g) * 6).to(lat_dtype)
    return lat, (torch.randn(rows, T, generator=g) * 0.5).to(lab_dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def _check_exact(out, lat, lab, idx, table, scale, seed, step, replica, p, tag):
    """mask, label, target against the numpy statement and the mix against train.mix_noise on the kernel's own draws: all ==."""
    target, label, nbad = R.gather(lat.numpy(), lab.numpy(), idx.numpy(), None if table is None else table.numpy(), scale)
    mask = R.label_mask(seed, step, replica, idx.numel(), p)
    label[mask] = 0
    got = {k: v.cpu() for k, v in out.items() if v is not None}
    assert np.array_equal(got["mask"].numpy().astype(bool), mask), tag
    assert np.array_equal(got["target"].numpy().view(np.int32), target.view(np.int32)), tag
    assert np.array_equal(got["label"].numpy().view(np.int32), label.view(np.int32)), tag
    assert int(got["bad"]) == nbad, tag
    B = idx.numel()
    want = mix_noise(got["target"].view(B, -1, 1, 1), got["noise_level64"], got["noise"].view(B, -1, 1, 1)).view(B, -1)
    assert torch.equal(_bits(got["x_noisy"]), _bits(want)), tag
    assert torch.equal(_bits(got["noise_level"]), _bits(got["noise_level64"].float())), tag
    nl = got["noise_level64"]
    assert bool(((nl > 0) & (nl < 1)).all()) and bool(torch.isfinite(got["noise"]).all()), tag


@pytest.mark.parametrize("lab_name", list(LAB_DTYPES))
@pytest.mark.parametrize("lat_name", list(LAT_DTYPES))
def test_gather_mask_and_mix_are_bitwise(lat_name, lab_name):
    """Every latent x label dtype at batch 5 and 128, C S S = 4 4 4 and 4 32 32 (the 16-byte path) and 3 3 3 (no multiple of 4: the element path, with
    Philox counters that straddle two samples), text_emb 768 and 10 (fp16 rows of 20 bytes: aligned to 4 at most), duplicated indices, clip_val 20."""
    dev = _dev()
    table = _table(20, 8.0)
    for case, (B, E, T) in enumerate([(5, 64, 768), (5, 4096, 10), (128, 64, 10), (128, 4096, 768), (5, 27, 10), (128, 27, 768)]):
        rows = 37                                                             # fewer rows than a batch of 128: duplicates are certain
        lat, lab = _source(rows, E, T, LAT_DTYPES[lat_name], LAB_DTYPES[lab_name], seed=case)
        idx = torch.randint(0, rows, (B,), generator=torch.Generator().manual_seed(100 + case))
        idx[1] = idx[0]; idx[-1] = rows - 1
        tab = table if lat_name == "u8" else None
        seed, step, replica = 0x123456789ABCDEF + case, (3 << 32) + 17 * case, case % 3
        out = _prepare(lat.to(dev), lab.to(dev), idx.to(dev), table=None if tab is None else tab.to(dev), scale=8.0, seed=seed, step=step, replica=replica)
        _check_exact(out, lat, lab, idx, tab, 8.0, seed, step, replica, 0.15, (lat_name, lab_name, B, E, T))


def test_unaligned_sources_take_the_element_path_and_give_the_same_bits():
    """Source rows that start 1 element into an allocation (the 4-element loads would be misaligned): same results as the aligned copy."""
    dev = _dev()
    for name, dt in LAT_DTYPES.items():
        lat, lab = _source(9, 64, 10, dt, torch.float16, seed=5)
        idx = torch.tensor([8, 0, 3, 3, 7])
        tab = _table().to(dev) if name == "u8" else None
        shifted = torch.zeros(9 * 64 + 1, dtype=dt, device=dev)
        shifted[1:] = lat.to(dev).reshape(-1)
        kw = dict(table=tab, seed=9, step=4, replica=1)
        a = _prepare(lat.to(dev), lab.to(dev), idx.to(dev), **kw)
        b = _prepare(shifted[1:].view(9, 64), lab.to(dev), idx.to(dev), **kw)
        assert shifted[1:].data_ptr() % 4 != 0 or dt != torch.uint8
        for k in ("x_noisy", "target", "noise", "label", "noise_level64", "mask"):
            assert torch.equal(a[k], b[k]), (name, k)
        _check_exact(b, lat, lab, idx, None if tab is None else tab.cpu(), 8.0, 9, 4, 1, 0.15, name)


@pytest.fixture(scope="module")
def big():
    """2^20 normals: batch 256 of 4 x 32 x 32 at seed 1234, step 7 (and batch 128 of the same call, for the prefix property)."""
    dev = _dev()
    lat, lab = _source(16, 4096, 10, torch.float16, torch.float32, seed=2)
    idx = torch.arange(256) % 16
    kw = dict(seed=1234, step=7, replica=0)
    full = _prepare(lat.to(dev), lab.to(dev), idx.to(dev), **kw)
    half = _prepare(lat.to(dev), lab.to(dev), idx[:128].to(dev), **kw)
    torch.cuda.synchronize()
    return dict(full={k: v.cpu() for k, v in full.items()}, half={k: v.cpu() for k, v in half.items()}, src=(lat, lab, idx), kw=kw)


def _ks(sample, cdf):
    x = np.sort(np.asarray(sample, dtype=np.float64))
    n = x.size
    f = cdf(x)
    return max(float((np.arange(1, n + 1) / n - f).max()), float((f - np.arange(n) / n).max()))


def test_noise_against_float64_box_muller_on_the_same_philox_bits(big):
    """|noise - float64 Box-Muller| <= 1e-5, the float64 side from the UNROUNDED uniforms ((r >> 8) + 0.5) 2^-24: logf / log1pf (1 ulp of |ln u| <= 17.3,
    i.e. 1e-6 / r in the radius r), the rounded sqrt, the angle's uniform rounded to fp32 (2 pi 2^-25 x radius <= 1.1e-6), sincospif and two fp32 products
    at radius <= 5.9 add up to about 4e-6.  Measured on an MI355X: 9.3e-7."""
    noise = big["full"]["noise"].numpy().reshape(-1).astype(np.float64)
    n = noise.size
    assert n == 1 << 20
    err = np.abs(noise - R.noise_f64(1234, 7, 0, n)).max()
    print(f"noise: max |fp32 - float64| {err:.3e}; max |noise| {np.abs(noise).max():.3f}")
    assert err <= 1e-5
    assert np.abs(noise).max() <= 5.9


def test_normals_pass_kolmogorov_smirnov(big):
    from scipy import stats
    noise = big["full"]["noise"].numpy().reshape(-1)
    d = _ks(noise, stats.norm.cdf)
    print(f"normals: n {noise.size}, KS {d:.3e} against {KS_ALPHA_001 / np.sqrt(noise.size):.3e}; mean {noise.mean():.2e}, var {noise.var():.5f}")
    assert d <= KS_ALPHA_001 / np.sqrt(noise.size)


@pytest.mark.parametrize("a,b", [(1, 2.5), (0.5, 0.5), (2, 5), (0.25, 8)])
def test_beta_draws_pass_kolmogorov_smirnov_and_follow_the_numpy_statement(a, b):
    """n = 65 536 noise levels (one row of four elements each).  Beside the KS bound: the kernel's double arithmetic and numpy's differ by roundings
    only -- a few ulp in ln Gamma, times up to |ln u| / a = 150 for the boosted shape 0.25, is 3e-14 in the exponent, a quarter of that in the level
    -- so the two agree to 1e-12 unless a rounding flipped an acceptance test (probability ~1e-15 per attempt)."""
    from scipy import stats
    dev = _dev()
    n = 65536
    lat, lab = _source(1, 4, 1, torch.float32, torch.float32)
    out = _prepare(lat.to(dev), lab.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), seed=1234, step=7, a=float(a), b=float(b))
    nl = out["noise_level64"].cpu().numpy()
    d = _ks(nl, stats.beta(a, b).cdf)
    ref = R.noise_level(1234, 7, 0, n, a, b)
    print(f"Beta({a}, {b}): KS {d:.3e} against {KS_ALPHA_001 / np.sqrt(n):.3e}; mean {nl.mean():.5f} (exact {a / (a + b):.5f}); "
          f"max |device - numpy| {np.abs(nl - ref).max():.2e}")
    assert (nl >= 0).all() and (nl <= 1).all()
    assert d <= KS_ALPHA_001 / np.sqrt(n)
    assert np.abs(nl - ref).max() <= 1e-12


def test_dropout_fraction_and_mask_bits_at_65536():
    dev = _dev()
    n = 65536
    lat, lab = _source(1, 4, 1, torch.float32, torch.float32)
    out = _prepare(lat.to(dev), lab.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), seed=1234, step=7)
    mask = out["mask"].cpu().numpy().astype(bool)
    frac = float(mask.mean())
    print(f"dropout fraction {frac:.4f} (4 sigma = {4 * np.sqrt(0.15 * 0.85 / n):.4f})")
    assert np.array_equal(mask, R.label_mask(1234, 7, 0, n, 0.15))
    assert abs(frac - 0.15) <= 4 * np.sqrt(0.15 * 0.85 / n)
    lab_out = out["label"].cpu().numpy().reshape(-1)
    assert (lab_out[mask] == 0).all() and (lab_out[~mask] == float(lab[0, 0])).all()
    for p, want in ((0.0, 0), (1.0, n)):                                      # u in [0, 1): nothing drops at 0, everything at 1
        assert int(_prepare(lat.to(dev), lab.to(dev), torch.zeros(n, dtype=torch.int64, device=dev), seed=1234, step=7, p=p)["mask"].sum()) == want


def test_same_arguments_same_bits_and_a_batch_is_a_prefix_of_a_larger_one(big):
    dev = _dev()
    lat, lab, idx = big["src"]
    again = _prepare(lat.to(dev), lab.to(dev), idx.to(dev), **big["kw"])
    for k, v in big["full"].items():
        assert torch.equal(again[k].cpu(), v), k
    full, half = big["full"], big["half"]
    for k in ("mask", "noise_level64", "noise_level", "noise", "x_noisy", "target", "label"):
        assert torch.equal(half[k], full[k][:128]), k


def test_step_replica_and_seed_each_change_every_stream(big):
    dev = _dev()
    lat, lab, idx = big["src"]
    base = big["half"]
    seen = [base]
    for change in (dict(step=8), dict(step=7 + (1 << 32)), dict(replica=1), dict(seed=1235), dict(seed=1234 + (1 << 32))):
        out = _prepare(lat.to(dev), lab.to(dev), idx[:128].to(dev), **dict(big["kw"], **change))
        out = {k: v.cpu() for k, v in out.items()}
        for other in seen:
            assert float((out["noise"] != other["noise"]).float().mean()) > 0.999, change
            assert bool((out["noise_level64"] != other["noise_level64"]).all()), change
            assert not torch.equal(out["mask"], other["mask"]), change
        seen.append(out)


def test_offsets_past_4_gib():
    """1 100 000 rows of 4 x 32 x 32 codes = 4.5 GB: byte offsets pass 2^31 at row 524 288 and 2^32 at row 1 048 576."""
    dev = _dev()
    rows, E = 1_100_000, 4096
    lat = torch.empty(rows, E, dtype=torch.uint8, device=dev)
    for i in range(0, rows, 100_000):                                         # (in slices: no fill kernel of the framework is asked for more than 2^32 elements)
        lat[i:i + 100_000] = torch.randint(0, 256, (min(100_000, rows - i), E), device=dev, dtype=torch.uint8)
    lab = torch.arange(rows, device=dev, dtype=torch.float32).view(rows, 1)
    table = _table().to(dev)
    idx = torch.tensor([rows - 1, 0, 524_287, 524_288, 1_048_575, 1_048_576, 1_048_577, rows - 2, 777_777, rows - 1], device=dev)
    out = _prepare(lat, lab, idx, table=table, seed=3, step=1, p=0.0)
    assert torch.equal(out["target"], table[lat[idx].long()])
    assert torch.equal(out["label"].view(-1), idx.float()) and int(out["bad"]) == 0
    B = len(idx)
    want = mix_noise(out["target"].cpu().view(B, E, 1, 1), out["noise_level64"].cpu(), out["noise"].cpu().view(B, E, 1, 1)).view(B, E)
    assert torch.equal(_bits(out["x_noisy"].cpu()), _bits(want))


@pytest.mark.parametrize("lat_name", list(LAT_DTYPES))
def test_bad_indices_are_counted_and_never_dereferenced(lat_name):
    """The sources are views into the MIDDLE of larger allocations whose margins hold sentinels: an index of -1 or `rows` that got through would read
    mapped memory and show as a sentinel value.  Such positions take row 0 and are counted."""
    dev = _dev()
    rows, E, T, margin = 6, 64, 10, 4
    dt = LAT_DTYPES[lat_name]
    lat, lab = _source(rows, E, T, dt, torch.float16, seed=8)
    if dt == torch.uint8:
        lat = lat.clamp(max=199)
    outer_lat = torch.full(((rows + 2 * margin), E), 255 if dt == torch.uint8 else 1000.0, dtype=dt, device=dev)
    outer_lab = torch.full(((rows + 2 * margin), T), 777.0, dtype=torch.float16, device=dev)
    outer_lat[margin:margin + rows] = lat.to(dev)
    outer_lab[margin:margin + rows] = lab.to(dev)
    tab = _table() if dt == torch.uint8 else None
    idx = torch.tensor([-1, rows, 0, rows - 1, -(1 << 40), 1 << 40, 2])
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    out = _prepare(outer_lat[margin:margin + rows], outer_lab[margin:margin + rows], idx.to(dev), table=None if tab is None else tab.to(dev), seed=2, step=3, p=0.0,
                   bad=bad)
    assert int(bad) == 4
    _check_exact(out, lat, lab, idx, tab, 8.0, 2, 3, 0, 0.0, lat_name)       # (the statement puts row 0 at the bad positions)
    row0 = out["target"][2]
    for pos in (0, 1, 4, 5):
        assert torch.equal(out["target"][pos], row0) and torch.equal(out["label"][pos], out["label"][2])
    assert float(out["target"].abs().max()) < 100 and float(out["label"].abs().max()) < 100          # no sentinel
    out = _prepare(outer_lat[margin:margin + rows], outer_lab[margin:margin + rows], torch.tensor([-1, rows, 0]).to(dev), table=None if tab is None else tab.to(dev),
                   bad=bad)
    assert int(bad) == 6                                                      # the cell accumulates: 4 + 2
    fresh = _prepare(outer_lat[margin:margin + rows], outer_lab[margin:margin + rows], torch.tensor([-1, rows, 0]).to(dev), table=None if tab is None else tab.to(dev))
    assert int(fresh["bad"]) == 2 and torch.equal(fresh["target"][0], fresh["target"][2]) and torch.equal(fresh["target"][1], fresh["target"][2])


# ---- through Trainer: the tiny g15 model at batch 4 ------------------------------------------------------------------------------------------
def _dataset(rows=16, lat_dtype=torch.uint8):
    lat, lab = _source(rows, 4 * 32 * 32, 768, lat_dtype, torch.float16, seed=31)
    return DeviceLatentDataset(lat.view(rows, 4, 32, 32), lab, device=_dev())


IDX = [[3, 7, 7, 15], [0, 1, 2, 3], [12, 4, 9, 4], [5, 6, 10, 11]]


def test_prepare_batch_is_the_entry_with_the_trainers_step_seed_and_rank():
    ds = _dataset()
    tr = _tiny(data_seed=77)
    tr.global_step = 5
    got = tr.prepare_batch(ds, IDX[0], debug=True)
    assert len(got) == 7 and tuple(got[0].shape) == (4, 4, 32, 32) and tuple(got[2].shape) == (4, 768) and got[6].dtype == torch.bool
    raw = _prepare(ds.latents.view(16, -1), ds.text_emb, torch.tensor(IDX[0], device=_dev()), table=ds.table, seed=77, step=5)
    for a, k in zip(got, ("x_noisy", "noise_level", "label", "target", "noise", "noise_level64", "mask")):
        assert torch.equal(a.reshape(raw[k].shape), raw[k].bool() if k == "mask" else raw[k]), k
    plain = tr.prepare_batch(ds, torch.tensor(IDX[0], device=_dev()))
    assert len(plain) == 4 and all(torch.equal(a, b) for a, b in zip(plain, got[:4]))
    assert not torch.equal(tr.prepare_batch(ds, IDX[0], step=6)[0], got[0])
    for bad in ([0, 16], [-1], [0.5]):
        with pytest.raises(IndexError):
            tr.prepare_batch(ds, bad)
    view = tr.bad_indices
    assert view.dim() == 0 and view.is_cuda and int(view) == 0
    tr.prepare_batch(ds, torch.tensor([0, 16, -1, 3], device=_dev()))             # a device index vector: the kernel's guard
    assert int(tr.bad_indices) == 2
    with pytest.raises(ValueError):
        tr.prepare_batch(DeviceLatentDataset(torch.zeros(4, 4, 16, 16), torch.zeros(4, 768), device=_dev()), [0])


@pytest.mark.parametrize("mode", ["eager", "graph", "host_copies"])
def test_train_step_from_equals_prepare_then_forward_backward_then_step(mode):
    """train_step_from against a second trainer handed prepare_batch's tensors: parameters, EMA and both Adam moments bit for bit after three steps --
    eagerly, under graph replay (step 1 eager, step 2 captures, step 3 replays) and with HOST copies of the tensors through the pinned staging path
    train_step uses."""
    ds = _dataset()
    graph = mode == "graph"
    a, b = _tiny(data_seed=5, use_graph=graph), _tiny(data_seed=5, use_graph=graph)
    for k in range(3):
        idx = torch.tensor(IDX[k], device=_dev())
        tensors = a.prepare_batch(ds, idx)                                    # what the step below is about to draw: (seed, rank, global_step) address it
        loss_a = a.train_step_from(ds, idx)
        if mode == "host_copies":
            staged = b._stage_batch(tuple(t.cpu() for t in tensors))
            loss_b, _ = b.forward_backward(*staged)
            b._release_stage()
        else:
            loss_b, _ = b.forward_backward(*tensors)
        b.optimizer_step()
        assert torch.equal(loss_a, loss_b) and np.isfinite(float(loss_a)), (mode, k)
        assert _same_bits(a, b), (mode, k)
    assert a.global_step == b.global_step == 3 and a.step == 3
    assert (a._graph is not None) == graph


def test_a_resumed_run_continues_the_noise_stream():
    ds = _dataset(lat_dtype=torch.float16)
    a = _tiny(data_seed=9)
    drawn, ckpt = [], None
    for k in range(4):
        if k == 2:
            ckpt = a.checkpoint()
        drawn.append(a.prepare_batch(ds, IDX[k], debug=True)[4:])
        a.train_step_from(ds, IDX[k])
    b = _tiny(data_seed=9)
    b.load_checkpoint(ckpt)
    assert b.global_step == 2
    for k in (2, 3):
        got = b.prepare_batch(ds, IDX[k], debug=True)[4:]
        assert all(torch.equal(x, y) for x, y in zip(got, drawn[k])), k
        b.train_step_from(ds, IDX[k])
    assert not torch.equal(drawn[2][0], drawn[3][0]) and b.global_step == 4

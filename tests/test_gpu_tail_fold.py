"""GPU: out_proj folded into the last block's down projection (tail_fold_kernel, tld_tail_fold_math.h).

With the fold the last block's 768-wide row x3 = x2 + hid Wd^T + bd is never formed: out = [x2 | hid] [Wout | Wout Wd]^T + (Wout bd + bo).  Tiny two-block
models, batch 3 (a partial workgroup), every branch of the kernel:

  c1geo   d 768, grid 16, patch 2 (16 patch features, NT 1), mlp_multiplier 4: the bench geometry
  d192    d 192, mlp_multiplier 2, grid 4: K = 576 (18 K-blocks over 8 waves: two waves without work), 16 rows per sample, the plain tail when unfolded
  d1024   d 1024, mlp_multiplier 4, grid 8: the largest K the engine admits (5120)
  p4      patch 4: 64 patch features, NT 4
  p1      patch 1: 4 patch features, NT 1 with 12 zero rows in the weight tile

Bounds.  EXACT, the project's bound for an fp32 result whose summation order alone differs from float64 (tests/test_gpu_forward_stages.py TAIL_TOL):
max |out - ref| <= 2e-5 max |ref|, ref the float64 evaluation of the folded formula from the engine's own blk1.ca / blk1.hid stages and the fp32 parameters,
Wd rounded to bf16.  Folded against unfolded (TLD_FOLD_TAIL=0, a fresh child process: the switch is read at engine creation): the one modelled
difference is the bf16 rounding of x3, half an ulp = 2^-9 relative per element, so per output |d| <= 2^-8 sum_k |Wout[f][k]| |x3[row][k]| + 2e-5 max |out|
(the factor 2 is headroom over that derivation); and the folded arm, which drops that rounding, has no larger rms error against float64.
Everything else is an equality: a sample's output does not depend on the batch it rides in (forward and CFG sampler, small and large launches: the
row tiles per workgroup follow the launch size), and a device weight refresh gives the bits of a fresh load.
"""
import gc
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import infer_stage_refs as F
import train_stage_refs as R
from test_gpu_forward_stages import _cfg, _inputs, _model
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

EXACT = 2e-5
BATCH = 3
SHAPES = {
    "c1geo": _cfg(768, 32, 2),
    "d192": _cfg(192, 8, 2, mult=2),
    "d1024": _cfg(1024, 16, 2),
    "p4": _cfg(256, 32, 2, patch=4),
    "p1": _cfg(256, 8, 2, patch=1),
}
BIT_FOLD, BIT_TAIL_MFMA, BIT_TAIL_PLAIN = 16, 45, 49


def _forward_stages(name):
    """One debug forward of shape `name` at BATCH in this process: out, the last block's ca / hid stages (fp32 arrays) and the launch paths."""
    kw = SHAPES[name]
    m = _model(kw)
    m.reserve(BATCH)
    m.set_debug(True)
    try:
        x, sigma, lab, _ = _inputs(kw, BATCH, 60)
        out = m(x.to(_dev()), sigma.to(_dev()), lab.to(_dev()))
        torch.cuda.synchronize()
        L = kw["n_layers"]
        got = {"out": m.read_stage("out"), "ca": m.read_stage(f"blk{L - 1}.ca"), "hid": m.read_stage(f"blk{L - 1}.hid"),
               "mlp": m.read_stage(f"blk{L - 1}.mlp"), "ret": out.float().cpu().numpy().reshape(BATCH, -1), "paths": np.array([m.debug_paths()], np.uint64)}
    finally:
        m.set_debug(False)
        del m
        gc.collect(); torch.cuda.empty_cache()
    return got


def child_main(path):
    """The unfolded arm (run with TLD_FOLD_TAIL=0 in the environment): every shape, saved as one npz."""
    out = {}
    for name in SHAPES:
        for k, v in _forward_stages(name).items():
            out[f"{name}.{k}"] = v
    np.savez(path, **out)


@pytest.fixture(scope="module")
def folded():
    return {name: _forward_stages(name) for name in SHAPES}


@pytest.fixture(scope="module")
def unfolded(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("tail_fold") / "unfolded.npz")
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_tail_fold as T; T.child_main(sys.argv[1])"
    r = subprocess.run([sys.executable, "-c", code, path], env=dict(os.environ, TLD_FOLD_TAIL="0"), capture_output=True, text=True, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(path)
    return {name: {k: z[f"{name}.{k}"] for k in ("out", "ca", "hid", "mlp", "ret", "paths")} for name in SHAPES}


_REF = {}


def _reference(name, run):
    """Float64, from the run's own stages: the folded formula's output image [B, img], x3 [M, d], and the per-output rounding budget sum_k |Wout| |x3|."""
    if name in _REF:
        return _REF[name]
    kw = SHAPES[name]
    dev = _dev()
    d, L, C, patch = kw["embed_dim"], kw["n_layers"], kw["n_channels"], kw["patch_size"]
    hid = d * kw["mlp_multiplier"]
    m = _model(kw)
    w = {k: v.to(dev).double() for k, v in m.state_dict().items() if v.dtype != torch.int64}
    del m
    p = f"{R.BLK}decoder_blocks.{L - 1}."
    Wout, bo = w[R.BLK + "out_proj.0.weight"], w[R.BLK + "out_proj.0.bias"]
    Wd, bd = F.bf16(w[p + "mlp.mlp.3.weight"].reshape(d, hid)), w[p + "mlp.mlp.3.bias"]
    ca, h = torch.from_numpy(run["ca"]).to(dev).double(), torch.from_numpy(run["hid"]).to(dev).double()
    feat = ca @ Wout.T + h @ (Wout @ Wd).T + (Wout @ bd + bo)                          # the folded formula, [M, pd]
    x3 = ca + h @ Wd.T + bd
    budget = x3.abs() @ Wout.abs().T
    img = lambda t: R.unpatchify(t.view(BATCH, -1, t.shape[-1]), C, patch).reshape(BATCH, -1)
    _REF[name] = (img(feat), x3, img(budget))
    return _REF[name]


def _paths(run):
    return int(run["paths"][0])


@pytest.mark.parametrize("name", list(SHAPES))
def test_folded_output_against_float64(folded, name):
    run = folded[name]
    kw = SHAPES[name]
    ref, x3, _ = _reference(name, run)
    out = torch.from_numpy(run["out"]).to(_dev()).double()
    assert bool(torch.isfinite(out).all())
    err = float((out - ref).abs().max() / ref.abs().max())
    print(f"{name}: folded out against float64, max |d| / max |ref| = {err:.3e} (bound {EXACT:.0e})")
    assert err <= EXACT, (name, err)
    assert np.array_equal(run["ret"], run["out"]), "the caller's output is the out stage"
    nt = (kw["n_channels"] * kw["patch_size"] ** 2 + 15) // 16
    p = _paths(run)
    assert p >> BIT_FOLD & 1 and p >> (BIT_TAIL_MFMA + nt - 1) & 1 and not p >> BIT_TAIL_PLAIN & 1, hex(p)
    # the debug stage of the last block's row: the unrounded fp32 row (EXACT against float64 of the same operands)
    mlp = torch.from_numpy(run["mlp"]).to(_dev()).double()
    e3 = float((mlp - x3).abs().max() / x3.abs().max())
    print(f"{name}: fp32 debug row against float64, max |d| / max |ref| = {e3:.3e}")
    assert e3 <= EXACT, (name, e3)


@pytest.mark.parametrize("name", list(SHAPES))
def test_folded_against_unfolded(folded, unfolded, name):
    fo, un = folded[name], unfolded[name]
    pu = _paths(un)
    assert not pu >> BIT_FOLD & 1, hex(pu)
    if SHAPES[name]["embed_dim"] % 128:
        assert pu >> BIT_TAIL_PLAIN & 1, hex(pu)                                      # the VALU tail: reached by the unfolded arm alone since the fold
    for st in ("ca", "hid"):                                                          # both arms are the same bits up to the fold's inputs
        assert np.array_equal(fo[st].view(np.uint32), un[st].view(np.uint32)), st
    ref, _, budget = _reference(name, fo)
    dev = _dev()
    of, ou = torch.from_numpy(fo["out"]).to(dev).double(), torch.from_numpy(un["out"]).to(dev).double()
    bound = 2.0 ** -8 * budget + EXACT * of.abs().max()
    worst = float(((of - ou).abs() / bound).max())
    rms = lambda t: float(((t - ref) ** 2).mean().sqrt() / (ref ** 2).mean().sqrt())
    rf, ru = rms(of), rms(ou)
    print(f"{name}: |folded - unfolded| / bound = {worst:.3e}; rel rms against float64: folded {rf:.3e}, unfolded {ru:.3e}")
    assert worst <= 1.0, (name, worst)
    assert rf <= ru, (name, rf, ru)


def _big_batch(rows_per_sample, tiles):
    """Samples whose rows reach launch_tail's large-launch form: 16 x tiles rows per workgroup once every CU has one."""
    cus = torch.cuda.get_device_properties(_dev()).multi_processor_count
    return -(-16 * tiles * cus // rows_per_sample)


@pytest.mark.parametrize("name,small,big", [("c1geo", 1, 5), ("c1geo", 1, 16), ("c1geo", 1, "RT4"), ("p4", 1, "RT2")])
def test_a_sample_does_not_depend_on_its_batch(name, small, big):
    """Sample 0 alone and inside a larger batch: bitwise equal.  (1, 16): one image, 16 workgroups of the folded kernel, against a 16-image batch;
    RT4 / RT2: the larger batch is the smallest that takes 4 (2, at more than 32 patch features) row tiles per workgroup."""
    kw = SHAPES[name]
    N = (kw["image_size"] // kw["patch_size"]) ** 2
    if big == "RT4":
        big = _big_batch(N, 4)
    elif big == "RT2":
        big = _big_batch(N, 2)
    dev = _dev()
    m = _model(kw)
    m.reserve(big)
    x, sigma, lab, _ = _inputs(kw, big, 70)
    x, sigma, lab = x.to(dev), sigma.to(dev), lab.to(dev)
    try:
        m.set_debug(True)
        m(x[:small], sigma[:small], lab[:small])
        assert m.debug_paths() >> BIT_FOLD & 1, "the small launch did not take the folded path"
        m.set_debug(False)
        a = m(x[:small], sigma[:small], lab[:small]).clone()
        b = m(x, sigma, lab).clone()
        assert bool(torch.isfinite(b).all()) and torch.equal(a[0], b[0])
        a2 = m(x[:small], sigma[:small], lab[:small]).clone()
        assert torch.equal(a, a2)
    finally:
        m.set_debug(False)
        del m
        gc.collect(); torch.cuda.empty_cache()


def test_sampler_sample_does_not_depend_on_its_batch():
    """A 4-step CFG sampler call (layer-0 sharing with its fan-out, the source-row table): request 0 alone and with four others, bitwise equal."""
    from transformer_latent_diffusion_amd import schedule
    kw = SHAPES["c1geo"]
    dev = _dev()
    m = _model(kw)
    m.reserve(10)
    x, _, lab, _ = _inputs(kw, 5, 71)
    x, lab = x.to(dev), lab.to(dev)
    co = schedule.step_coefficients(schedule.noise_schedule(4, 1), True)
    try:
        one = m.sample_latents(x[:1], lab[:1], co, 3.0).clone()
        five = m.sample_latents(x, lab, co, 3.0).clone()
        assert bool(torch.isfinite(five).all()) and torch.equal(one[0], five[0])
    finally:
        del m
        gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["c1geo", "p1"])
def test_refresh_gives_the_bits_of_a_fresh_load(name):
    """load_flat with other weights rebuilds the folded operand on the device (refresh_tail_fold_kernel): out is bitwise what an engine that loaded those
    weights through the host path gives, and two runs are bitwise equal."""
    from dataclasses import asdict
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, flatten_state_dict
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    kw = SHAPES[name]
    cfg = DenoiserConfig(**kw)
    dev = _dev()
    sds = [{k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, seed).items()} for seed in (0, 1)]
    x, sigma, lab, _ = _inputs(kw, BATCH, 72)
    x, sigma, lab = x.to(dev), sigma.to(dev), lab.to(dev)
    h = Denoiser(**asdict(cfg)).to(dev)
    h.load_state_dict(sds[1])
    h.reserve(BATCH)
    dm = Denoiser(**asdict(cfg)).to(dev)
    dm.load_state_dict(sds[0])
    dm.reserve(BATCH)
    try:
        before = dm(x, sigma, lab).clone()
        dm.load_flat(flatten_state_dict(sds[1], cfg).to(dev))
        after = dm(x, sigma, lab).clone()
        again = dm(x, sigma, lab).clone()
        fresh = h(x, sigma, lab).clone()
        assert bool(torch.isfinite(fresh).all()) and not torch.equal(before, after)
        assert torch.equal(after, fresh) and torch.equal(after, again)
    finally:
        del h, dm
        gc.collect(); torch.cuda.empty_cache()

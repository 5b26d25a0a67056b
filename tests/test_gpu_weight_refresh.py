"""GPU: the device weight refresh (tld_engine_refresh_weights, Denoiser.load_flat, Trainer.sync_denoiser / eval_generate).

A refresh must leave exactly the engine a fresh load of the same values builds, so every comparison here is an equality: engine H is a fresh
Denoiser with load_state_dict(B) (tld_engine_load_tensor + tld_engine_finalize_weights), engine D held weights A, ran a forward, and took B
through load_flat.  Both run the refresh kernels, so what those compute is held against an independent statement: every weight image of either
engine, read through the stage hook, must have the bits of the numpy restatement in weight_image_refs.py.  With the stage hook on, EVERY stage
of a forward -- the weight images included -- must have the same bits in both engines, poison and all; with it off, the forward and a CFG
sampler must return equal tensors.  Weights: synth_state_dict, seed 0 = "A", seed 1 = "B"; two blocks, model batch 3."""
import ctypes as C
import os
from dataclasses import asdict

import numpy as np
import pytest
import torch

from test_gpu_parity import _dev
from weight_image_refs import BLOCK_IMAGES, GLOBAL_IMAGES, as_read, engine_mode, weight_images
from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator, TrainConfig, Trainer, _lib, flatten_state_dict, schedule, weights

pytestmark = pytest.mark.gpu

BATCH = 3


def _cfg(d, image, patch=2, C_=4):
    return DenoiserConfig(image_size=image, noise_embed_dims=256, patch_size=patch, embed_dim=d, dropout=0, n_layers=2, text_emb_size=768, n_channels=C_)


# name -> (config, environment at engine creation, GEMM dtype, low-latency class): each the smallest shape that reaches one branch of finalize
CASES = {
    "d768_256tok": (_cfg(768, 32), {}, "bf16", 0),                                                # both folds, packed fused-QKV rows, fused 16 x 16 depthwise taps
    "d768_256tok_no_folds": (_cfg(768, 32), {"TLD_FOLD_LN1": "0", "TLD_FOLD_LN3": "0"}, "bf16", 0),      # the plain bf16 operands
    "d768_256tok_two_kernel_qkv": (_cfg(768, 32), {"TLD_FUSE_QKV_ATTN": "0"}, "bf16", 0),                # the fold without the packing
    "d192_64tok": (_cfg(192, 16), {}, "bf16", 0),
    "d256_64tok": (_cfg(256, 16), {}, "bf16", 0),
    "d1024_64tok": (_cfg(1024, 16), {}, "bf16", 0),
    "d768_256tok_fp8": (_cfg(768, 32), {}, "fp8", 0),                                             # the three quantised images
    "d768_256tok_low_latency": (_cfg(768, 32), {}, "bf16", 1),
    "d384_256tok_low_latency": (_cfg(384, 32), {}, "bf16", 1),
    "d192_patch4": (_cfg(192, 32, patch=4), {}, "bf16", 0),                                       # patch_dim 64: hi / lo splits and the [pd, d] transpose at one end
    "d192_patch1": (_cfg(192, 8, patch=1), {}, "bf16", 0),                                        # ... patch_dim 4: at the other
}

_SD = {}


def _sd(cfg, seed):
    key = (tuple(sorted(asdict(cfg).items())), seed)
    if key not in _SD:
        sd = {k: torch.from_numpy(np.array(v)) for k, v in weights.synth_state_dict(cfg, seed).items()}
        _SD[key] = (sd, flatten_state_dict(sd, cfg))
    return _SD[key]


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _model(case, seed, batch=BATCH):
    """A Denoiser of the case holding the weights of `seed` through load_state_dict, its engine built (the switches are read at tld_engine_create)."""
    cfg, env, dtype, lowlat = CASES[case]
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict(_sd(cfg, seed)[0])
    if dtype != "bf16":
        m.set_gemm_dtype(dtype)
    if lowlat:
        m.set_low_latency(lowlat)
    _with_env(env, lambda: m.reserve(batch))
    return m


def _inputs(cfg, B=BATCH, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, cfg.n_channels, cfg.image_size, cfg.image_size, generator=g)
    sigma = torch.rand(B, 1, generator=g) * 0.9 + 0.05
    lab = torch.randn(B, cfg.text_emb_size, generator=g) * 0.5
    lab[B - 1] = 0
    return x.to(_dev()), sigma.to(_dev()), lab.to(_dev())


def _stage_names(cfg):
    """Every name the stage hook of a forward can hold (include/tld_hip.h); which of them exist depends on the engine's mode."""
    names = ["tokens0", "out", "cond.sin", "cond.h1", "cond.pre", "cond.y", "cond.kv", "cond.wq", "cond.bwq"] + GLOBAL_IMAGES
    per_block = ["x_in", "ln1", "xn1", "qk", "vt", "att", "sa", "ca", "stats", "xn3", "hid_pre", "hid", "splitk", "mlp", "a8_qkv.q", "a8_qkv.s", "a8_up.q",
                 "a8_up.s", "a8_down.q", "a8_down.s", "wqkv", "wup", "wdown", "qkv_c1", "qkv_b1", "up_c1", "up_b1"] + BLOCK_IMAGES
    return names + [f"blk{i}.{n}" for i in range(cfg.n_layers) for n in per_block]


def _stages(m, cfg, inputs):
    """One debug forward: {name: raw bits of the stage} for every stage that exists, and the output."""
    m.set_debug(True)
    out = m(*inputs).clone()
    got = {}
    for n in _stage_names(cfg):
        try:
            m.stage_shape(n)
        except RuntimeError:
            continue
        got[n] = np.ascontiguousarray(m.read_stage(n)).view(np.uint32)
    m.set_debug(False)
    return got, out


_REF = {}


def _images(case, seed):
    """{stage name: bits} of every weight image an engine of the case holds with the weights of `seed`, from the numpy restatement."""
    if (case, seed) not in _REF:
        cfg, env, dtype, _ = CASES[case]
        ref = weight_images(_sd(cfg, seed)[0], cfg, engine_mode(cfg, env, dtype))
        _REF[case, seed] = {n: as_read(a).view(np.uint32) for n, a in ref.items()}
    return _REF[case, seed]


def _assert_same_engine_state(h, d, cfg, what, ref):
    """Requirements 2 and 3: every stage of a debug forward has the same bits in both engines; with debug off the forward and the end latent of a
    4-level CFG sampler are equal.  `ref` (_images): every weight image either engine holds has the bits of the restatement, and no other exists."""
    inputs = _inputs(cfg)
    sh, oh = _stages(h, cfg, inputs)
    sd_, od = _stages(d, cfg, inputs)
    assert set(sh) == set(sd_), (what, set(sh) ^ set(sd_))
    for who, got in (("load_state_dict", sh), ("load_flat", sd_)):
        held = {n for n in got if "img." in n or n.split(".")[-1] in ("wqkv", "wup", "wdown", "qkv_c1", "qkv_b1", "up_c1", "up_b1")}
        assert held == set(ref), (what, who, held ^ set(ref))
        wrong = [n for n in ref if got[n].shape != ref[n].shape or not np.array_equal(got[n], ref[n])]
        assert not wrong, (what, who, wrong)
    operands = [n for n in sh if n.split(".")[-1] in ("wqkv", "wup", "wdown")]
    assert len(operands) == 3 * cfg.n_layers and "tokens0" in sh and "out" in sh, (what, sorted(sh))
    differ = [n for n in sh if sh[n].shape != sd_[n].shape or not np.array_equal(sh[n], sd_[n])]
    assert not differ, (what, differ)
    assert torch.equal(oh, od), what
    assert torch.equal(h(*inputs), d(*inputs)), what
    co = schedule.step_coefficients(schedule.noise_schedule(4, 1), True)      # four levels
    assert co.shape[0] == 4
    x, _, lab = inputs
    assert torch.equal(h.sample_latents(x[:1], lab[:1], co, 4.5, 0.1, 0.1), d.sample_latents(x[:1], lab[:1], co, 4.5, 0.1, 0.1)), what


def _refreshed(case, first=0, then=1, on_device=True):
    """Engine D: holds `first`, reserved, ran one forward, then load_flat(`then`).  Requirement 1: the engine handle is the same one."""
    cfg = CASES[case][0]
    d = _model(case, first)
    d(*_inputs(cfg))
    handle, cap = d._engine.value, d._engine_batch
    flat = _sd(cfg, then)[1]
    d.load_flat(flat.to(_dev()) if on_device else flat)
    assert d._engine.value == handle and d._engine_batch == cap
    return d


@pytest.mark.parametrize("case", list(CASES))
def test_refreshed_engine_equals_host_loaded_engine(case):
    cfg = CASES[case][0]
    h = _model(case, 1)
    d = _refreshed(case)
    L = _lib.lib()
    assert L.tld_engine_param_count(d._engine) == weights.param_count(cfg) == d.param_count
    wb = L.tld_engine_weight_bytes(d._engine)
    assert wb == L.tld_engine_weight_bytes(h._engine)
    _assert_same_engine_state(h, d, cfg, case, _images(case, 1))
    if case == "d768_256tok":       # no residue: back to A on the refreshed engine (from a HOST vector this time) = a fresh host-loaded A
        handle = d._engine.value
        d.load_flat(_sd(cfg, 0)[1])
        assert d._engine.value == handle and L.tld_engine_weight_bytes(d._engine) == wb
        _assert_same_engine_state(_model(case, 0), d, cfg, case + " back to A", _images(case, 0))


def test_state_dict_and_rebuild_after_load_flat():
    """state_dict() and parameters() after load_flat return B, angular_speeds stays; a reserve of a larger batch rebuilds the engine from B."""
    case = "d256_64tok"
    cfg = CASES[case][0]
    sd_b = _sd(cfg, 1)[0]
    d = _model(case, 0)
    ang = d.state_dict()["fourier_feats.0.angular_speeds"] * 1.5          # (not the default: it must survive the load)
    d.load_state_dict({"fourier_feats.0.angular_speeds": ang}, strict=False)
    d.reserve(BATCH)
    d(*_inputs(cfg))
    d.load_flat(_sd(cfg, 1)[1].to(_dev()))
    got = d.state_dict()
    for k in sd_b:
        assert torch.equal(got[k], ang if k == "fourier_feats.0.angular_speeds" else sd_b[k]), k
    for p, k in zip(d.parameters(), weights.param_layout(cfg)):
        assert torch.equal(p, sd_b[k]), k
    h = Denoiser(**asdict(cfg)).to(_dev())
    h.load_state_dict(dict(sd_b, **{"fourier_feats.0.angular_speeds": ang}))
    inputs = _inputs(cfg)
    assert torch.equal(h(*inputs), d(*inputs))
    old = d._engine.value
    d.reserve(16)
    assert d._engine_batch >= 16 and old is not None       # (rebuilt: the first engine held 8 samples)
    big = _inputs(cfg, 16, 9)
    assert torch.equal(h(*big), d(*big))
    assert torch.equal(h(*inputs), d(*inputs))


def _quantiser_rows(K, rows=8, seed=3):
    """fp32 [rows, K] of 32-element blocks: the shapes of block a quantiser can get wrong, then normal values over 2^-30 .. 2^20."""
    rng = np.random.default_rng(seed)
    nblk = rows * K // 32
    x = (rng.choice([-1.0, 1.0], (nblk, 32)) * (1.0 + rng.random((nblk, 32))) * np.exp2(rng.integers(-30, 20, (nblk, 1)) - rng.integers(0, 12, (nblk, 32)))).astype(np.float32)
    b = 0
    x[b] = 0.0; b += 1                                                                          # all zero
    x[b] = 0.0; x[b, 5] = -0.0; b += 1
    for e in (-135, -140, -149):                                                                # the maximum is subnormal AFTER scaling (X stops at 2^-127)
        x[b] = (rng.integers(-3, 4, 32) * np.exp2(float(e))).astype(np.float32); x[b, 7] = np.exp2(float(e)) * 3; b += 1
    # exactly halfway between two codes after scaling (X = 1: the maximum 300 sits in [256, 512)), both parities, normal and subnormal codes, both signs
    steps = np.concatenate([np.arange(1, 16, 2) * 2.0 ** -10, (np.arange(8, 16) + 0.5) * 2.0 ** -9, (np.arange(8, 16) + 0.5) * 2.0 ** -3,
                            (np.arange(8, 15) + 0.5) * 2.0 ** 4])
    for sgn in (1.0, -1.0):
        x[b] = 0.0; x[b, :31] = (sgn * steps[:31]).astype(np.float32); x[b, 31] = 300.0; b += 1
    x[b] = 0.0; x[b, :4] = [447.9, 448.0, 460.0, -511.0]; x[b, 4] = 256.0; b += 1               # saturation (511 scales to 511 > 448)
    for pos in range(32):                                                                       # the maximum at each of the 32 positions
        x[b] = (rng.standard_normal(32) * 0.01).astype(np.float32); x[b, pos] = -7.0 if pos % 2 else 7.0; b += 1
    assert b <= nblk
    return x.reshape(rows, K)


@pytest.mark.parametrize("K", [256, 3072])
def test_fp32_device_quantiser_equals_the_host_quantiser(K):
    L = _lib.lib()
    x = _quantiser_rows(K)
    rows = x.shape[0]
    q_ref, s_ref = np.zeros((rows, K), np.uint8), np.zeros((K // 128, rows, 4), np.uint8)
    _lib.check(L.tld_debug_quant_mx8_host(x.ctypes.data_as(C.POINTER(C.c_float)), rows, K, q_ref.ctypes.data, s_ref.ctypes.data), "quant_mx8_host")
    assert len(np.unique(q_ref)) > 200                                                          # (the inputs reach most of the code space)
    xd = torch.from_numpy(x).to(_dev())
    q = torch.full((rows, K), 0xAA, dtype=torch.uint8, device=_dev())
    s = torch.full((K // 128, rows, 4), 0xAA, dtype=torch.uint8, device=_dev())
    _lib.check(L.tld_debug_quant_mx8_f32(xd.data_ptr(), q.data_ptr(), s.data_ptr(), rows, K, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "quant_mx8_f32")
    torch.cuda.synchronize()
    bad = np.argwhere(q.cpu().numpy() != q_ref)
    assert bad.size == 0, [(tuple(i), float(x[tuple(i)]), int(q.cpu().numpy()[tuple(i)]), int(q_ref[tuple(i)])) for i in bad[:8]]
    assert np.array_equal(s.cpu().numpy(), s_ref)


TRAIN_CFG = _cfg(256, 16)


def _train_batches(n, B=8, seed=21):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, 4, 16, 16, generator=g) * 0.5, torch.randn(B, 768, generator=g) * 0.5) for _ in range(n)]


def _step(tr, batch, i):
    return tr.train_step(batch[0], batch[1], np_rng=np.random.default_rng(100 + i), generator=torch.Generator().manual_seed(200 + i))


def _host_loaded(sd):
    m = Denoiser(**asdict(TRAIN_CFG)).to(_dev())
    m.load_state_dict({k: v.detach().cpu() for k, v in sd.items()}, strict=False)
    return m.reserve(BATCH)


@pytest.mark.parametrize("graph", [False, True])
def test_live_trainer_sync(graph):
    """After training steps the synced denoiser equals a host-loaded one (EMA and live weights), again after one more step; an evaluation in the
    middle changes no bit of the following training step (eager, and under the trainer's graph replay)."""
    batches = _train_batches(5)
    inputs = _inputs(TRAIN_CFG)
    mk = lambda: Trainer(TRAIN_CFG, TrainConfig(batch_size=8, lr=1e-3, alpha=0.9), device=_dev(), init_seed=4, max_batch=8, use_graph=graph)
    tr, ref = mk(), mk()
    for i in range(3):
        _step(tr, batches[i], i)
        _step(ref, batches[i], i)
    assert (tr._graph is not None) == graph
    den = tr.make_denoiser(BATCH)
    live = tr.make_denoiser(BATCH, weights="live")
    handle = den._engine.value
    for i in (3, 4):
        assert tr.sync_denoiser(den) is den and den._engine.value == handle
        assert torch.equal(den(*inputs), _host_loaded(tr.ema_state_dict())(*inputs)), i
        tr.sync_denoiser(live, weights="live")
        assert torch.equal(live(*inputs), _host_loaded(tr.state_dict())(*inputs)), i
        assert not torch.equal(den(*inputs), live(*inputs))
        la, lb = _step(tr, batches[i], i), _step(ref, batches[i], i)        # a training step after the evaluation = the step of a trainer that never evaluated
        assert torch.equal(la, lb) and torch.equal(tr.params, ref.params) and torch.equal(tr.ema, ref.ema), i
        assert tr.global_step == ref.global_step and tr.step == ref.step


def test_eval_generate_equals_the_generator_on_a_host_loaded_ema():
    batches = _train_batches(2)
    tr = Trainer(TRAIN_CFG, TrainConfig(batch_size=8, lr=1e-3, alpha=0.9), device=_dev(), init_seed=4, max_batch=8)
    labels = torch.randn(8, 768, generator=torch.Generator().manual_seed(1)) * 0.5

    def reference():
        m = Denoiser(**asdict(TRAIN_CFG)).to(_dev())
        m.load_state_dict(tr.ema_state_dict())
        return DiffusionGenerator(m, None, _dev(), torch.float32).generate_latents(labels=torch.repeat_interleave(labels, 2, dim=0), num_imgs=16, class_guidance=4.5,
                                                                                  seed=10, n_iter=6, exponent=1, sharp_f=0.1, img_size=TRAIN_CFG.image_size)
    _step(tr, batches[0], 0)
    step, gstep = tr.step, tr.global_step
    first = tr.eval_generate(labels, n_iter=6)                         # builds the cached denoiser
    assert first.shape == (16, 4, 16, 16) and torch.equal(first, reference())
    den = tr._eval_den
    handle = den._engine.value
    _step(tr, batches[1], 1)
    second = tr.eval_generate(labels, n_iter=6)                        # syncs it in place
    assert tr._eval_den is den and den._engine.value == handle
    assert torch.equal(second, reference()) and not torch.equal(first, second)
    assert (tr.step, tr.global_step) == (step + 1, gstep + 1)


def test_refusals_change_nothing():
    case = "d192_64tok"
    cfg = CASES[case][0]
    d = _model(case, 0)
    inputs = _inputs(cfg)
    before = d(*inputs).clone()
    flat = _sd(cfg, 1)[1].to(_dev())
    with pytest.raises(ValueError):
        d.load_flat(flat[:-1])
    with pytest.raises(TypeError):
        d.load_flat(flat.double())
    L = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.tld_engine_refresh_weights(d._engine, C.c_void_p(flat.data_ptr()), flat.numel() - 1, stream) == 3        # TLD_ERR_SHAPE
    assert b"elements" in L.tld_last_error()
    assert torch.equal(d(*inputs), before)
    # before finalize: TLD_ERR_STATE
    c = asdict(cfg)
    cc = _lib.TldConfig(c["image_size"], c["noise_embed_dims"], c["patch_size"], c["embed_dim"], c["n_layers"], c["text_emb_size"], c["n_channels"],
                        c["mlp_multiplier"], BATCH, _dev().index)
    h = C.c_void_p()
    _lib.check(L.tld_engine_create(C.byref(cc), C.byref(h)), "tld_engine_create")
    try:
        assert L.tld_engine_param_count(h) == flat.numel()
        assert L.tld_engine_refresh_weights(h, C.c_void_p(flat.data_ptr()), flat.numel(), stream) == 4                # TLD_ERR_STATE
    finally:
        L.tld_engine_destroy(h)
    tr = Trainer(TRAIN_CFG, device=_dev(), init_seed=4, max_batch=8, keep_ema=False)
    with pytest.raises(RuntimeError):
        tr.make_denoiser(BATCH)
    den = tr.make_denoiser(BATCH, weights="live")
    with pytest.raises(RuntimeError):
        tr.sync_denoiser(den, weights="ema")
    with pytest.raises(RuntimeError):
        tr.eval_generate(torch.zeros(8, 768), n_iter=6)
    with pytest.raises(ValueError):
        tr.sync_denoiser(den, weights="best")

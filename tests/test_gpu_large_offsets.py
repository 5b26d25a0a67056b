"""GPU: the denoiser engine, the sampler, the training engine and their raw-buffer kernel hooks at sizes whose activation buffers pass 2 GiB, up to the top of
the range the engines accept (just below 4 GiB per buffer): every offset of DESIGN.md section 7.19's table that is not 64-bit, executed above 2^31.

Method: equality.  A large batch is built from P = 3 distinct samples (one with an all-zero label, distinct noise levels) laid out by a non-periodic map of the
sample index (a multiplicative hash mod 3), so that an address that wrapped, or a signed product that went negative, cannot land on a row holding the same
values.  Every output row of the large call must equal, bit for bit, the same sample run three at a time on the same engine -- the project already holds that a
sample's output depends neither on the batch it rides in nor on its position (tests/test_gpu_tail_fold.py, test_gpu_requests.py, test_gpu_eval_loss.py), and the
three samples themselves are held against float64 by tests/test_gpu_forward_stages.py, test_gpu_train_stages.py and the hooks' own files at these configurations:
that is the anchor of truth, this file adds none.  A failure names the mismatching samples, the last sample and the samples that straddle 2^31 bytes of each
activation buffer.  Everything is compared on the device; only counts and the first indices come back.

The training backward is made local by a sparse loss: target = pred everywhere except on four active samples (sample 0, the last, and the two that straddle
2^31 bytes of the [M, hid] and [M, 3 d] buffers; more where the batch is not four times a power of two), the inactive samples' losses are asserted to be exactly 0.0, and
the flat gradient times batch / active samples (a power of two) must match the gradient of the active samples alone within the project's EXACT bound for fp32 results whose summation order alone differs,
|a - b| <= 2e-5 max |b| per tensor (tests/test_gpu_train_stages.py).  A kernel that reads a wrong row past 2 GiB shows as an error of order one.

GPU cases stay strictly inside what the engines and hooks accept; beyond it only refusals are asked, which launch nothing (tests/test_large_offsets_host.py and
tests/test_body_plan_host.py hold them without a device).  The stage hook is off throughout (its snapshots would multiply the memory); the launch paths of a case
are the engine's plan, restated by tests/body_plan_ref.py.  Each test states the device bytes it needs and skips only when torch.cuda.mem_get_info() shows less.

The sampler: one call of the request entries carries at most 1024 conditioning rows (kMaxRequestCondRows), so 1365 requests cannot ride
in one generate_latents_requests call.  That call is asserted as a refusal; 2730 model rows run through the uniform entry, the request entry at 1000 requests.

What running found (profiles/large_offsets_gpu_tests.txt): no kernel fault and no mismatch -- every case passed on its first execution, the gradients at no more
than 0.03 of the EXACT bound.  What was wrong was in the guards, found by reading and closed before the first large run: tld_engine_create
admitted engines whose first forward launch_gemm refused (more than 2^24 rows at narrow widths) or no attention launch could carry (more than 65 535 samples);
tld_train_create admitted 2715 ... 2730 samples at d 768, grid 16, where the transposed weight-gradient operands T1 / T2 pass 4 GiB; tld_debug_dwconv_gelu launched the
row-streaming kernel, whose byte offset wraps at 4 GiB, at any size.
"""
import ctypes as C
import gc
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

import body_plan_ref as BP
from test_gpu_forward_stages import _cfg, _model, _with_env
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = 2e-5
GIB = 1 << 30
P = 3


def _record(line):
    print("\n[large offsets] " + line)
    path = os.environ.get("TLD_LARGE_OFFSETS_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _need_free(nbytes, what):
    free, _ = torch.cuda.mem_get_info(_dev())
    if free < nbytes:
        pytest.skip(f"{what} needs {nbytes} bytes ({nbytes / GIB:.1f} GiB) of free device memory, the device has {free} ({free / GIB:.1f} GiB) free")


def _free():
    gc.collect()
    torch.cuda.empty_cache()


def replica_map(B):
    """Sample index -> which of the P samples it carries: a multiplicative hash mod P (no period: for any shift s the map and its shift differ at two samples in
    three), with sample 0 -> 0 and every replica present."""
    i = torch.arange(B, dtype=torch.int64)
    idx = (((i * 2654435761) & 0xFFFFFFFF) >> 11) % P
    assert len(torch.unique(idx)) == P
    return idx


def straddlers(B, per_sample_bytes):
    """{buffer: the sample whose rows hold byte 2^31 of that buffer} for the buffers that reach it."""
    return {name: (1 << 31) // per for name, per in per_sample_bytes.items() if (1 << 31) // per < B}


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def mismatches(big, ref, idx, chunk=256):
    """Samples of `big` [B, ...] whose bits differ from ref[idx[b]] (device tensors): (count, the first indices)."""
    bad = []
    for s in range(0, big.shape[0], chunk):
        e = min(s + chunk, big.shape[0])
        bad.append((_bits(big[s:e]) != _bits(ref[idx[s:e]])).flatten(1).any(1))
    bad = torch.cat(bad).nonzero().flatten()
    return int(bad.numel()), bad[:8].tolist()


def _three(kw, seed):
    """Three distinct samples: x, distinct noise levels, labels of which sample 1's is all zero."""
    g = torch.Generator().manual_seed(seed)
    S, Cn = kw["image_size"], kw["n_channels"]
    x = torch.randn(P, Cn, S, S, generator=g)
    sigma = torch.tensor([[0.15], [0.5], [0.85]])
    lab = torch.randn(P, 768, generator=g) * 0.5
    lab[1] = 0
    return x, sigma, lab


# ---- 1. the inference engine ---------------------------------------------------------------------------------------------------------------------------------------
# name: (config, max_batch, environment at tld_engine_create, operand type).  Two blocks: block 0 runs the down projection GEMM, block 1 the folded tail.
ENGINES = {
    "c1_2gib": (_cfg(768, 32, 2), 1400, {}, "bf16"),                              # fused QKV + attention on pair tiles, fused 16 x 16 up, 384-wide down, tail fold: hid 2.05 GiB
    "c1_top": (_cfg(768, 32, 2), 2730, {}, "bf16"),                               # the same at the top of the range: 3.999 GiB (2731 is refused)
    "g32": (_cfg(768, 64, 2), 682, {}, "bf16"),                                   # LayerNorm-1 fold + chunked attention, fused 32 x 32 up + seam kernel: 3.996 GiB
    "g32_stream": (_cfg(768, 64, 2), 682, {"TLD_FUSE_DWCONV": "0"}, "bf16"),      # up-projection alone + the row-streaming depthwise kernel and its 32-bit ooff
    "g64": (_cfg(768, 128, 2), 170, {}, "bf16"),                                  # 4096 tokens: 3.98 GiB
    "w256": (_cfg(256, 32, 2), 8190, {}, "bf16"),                                 # narrow rows, many of them: plain QKV, cross_row_mfma<1>, M = 2 096 640 rows
    "fp8": (_cfg(768, 128, 2), 170, {}, "fp8"),                                   # a8 / as8 and mx8_scale_index, the quantising stream kernel: the largest the guard admits
    "v384": (_cfg(384, 16, 2, patch=1, C=8, mult=2), 10922, {}, "bf16"),          # mlp_multiplier 2: q|k as large as hid, M = 2 796 032 rows: the largest the guard admits
}


def _engine_bytes(kw, max_batch, fp8):
    g = kw["image_size"] // kw["patch_size"]
    M, d = max_batch * g * g, kw["embed_dim"]
    hid = d * kw["mlp_multiplier"]
    act = M * (5 * d * 2 + 2 * d * 2 + 2 * hid * 2 + hid + (hid + hid // 32 if fp8 else 0)) + (M + 256) * 9 * 8      # x, x_half, xn, vt, att | qk | hid1, hid2 | seam | a8, as8
    io = 8 * max_batch * kw["n_channels"] * kw["image_size"] ** 2 * 4
    return act + io + 2 * GIB


def _buffers(kw):
    g = kw["image_size"] // kw["patch_size"]
    N, d = g * g, kw["embed_dim"]
    return {"hid": N * d * kw["mlp_multiplier"] * 2, "qk": N * 2 * d * 2, "x": N * d * 2}


@pytest.mark.parametrize("name", list(ENGINES))
def test_forward_at_large_batch_equals_the_samples_three_at_a_time(name):
    kw, B, env, dtype = ENGINES[name]
    need = _engine_bytes(kw, B, dtype == "fp8")
    _need_free(need, f"engine {name}")
    t0 = time.time()
    dev = _dev()
    plan = BP.Engine(NS(**{k: v for k, v in kw.items() if k != "dropout"}), B, env, torch.cuda.get_device_properties(dev).multi_processor_count)
    assert plan.refusal == "", plan.refusal
    if dtype == "fp8":
        assert plan.op("d1") == ""
    m = _model(kw)
    if dtype == "fp8":
        m.set_gemm_dtype("fp8")
    try:
        _with_env(env, lambda: m.reserve(B))
        x, sigma, lab = (t.to(dev) for t in _three(kw, 200 + len(name)))
        ref = m(x, sigma, lab).clone()
        assert bool(torch.isfinite(ref).all()) and not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2]) and not torch.equal(ref[0], ref[2])
        idx = replica_map(B).to(dev)
        big = m(x[idx], sigma[idx], lab[idx])
        torch.cuda.synchronize()
        n_bad, first = mismatches(big, ref, idx)
        named = dict(straddlers(B, _buffers(kw)), last=B - 1)
        g = kw["image_size"] // kw["patch_size"]
        hid_bytes = B * g * g * kw["embed_dim"] * kw["mlp_multiplier"] * 2
        again = m(x, sigma, lab)
        torch.cuda.synchronize()
        paths = {k: int(v) for k, v in vars(plan.p).items() if k in ("fp8", "fold_ln1", "fold_ln3", "fused_qa", "pair", "fuse_dw", "seam", "fold_tail", "ln_mx8", "cross_mx8", "dw_mx8")}
        _record(f"forward {name}: max_batch {B}, rows {B * g * g}, hidden bytes {hid_bytes} ({hid_bytes / GIB:.3f} GiB), needs {need / GIB:.1f} GiB; plan {paths}; "
                f"mismatching samples {n_bad} of {B}; batch 3 afterwards equal {bool(torch.equal(again, ref))}; {time.time() - t0:.1f} s")
        assert n_bad == 0, (f"{name}: {n_bad} of {B} samples differ from the sample run three at a time; first {first}; the samples that straddle 2^31 bytes of a buffer "
                            f"and the last one: {named}")
        assert torch.equal(again, ref), f"{name}: a batch of 3 after the large call gives other bits"
    finally:
        del m
        _free()


def test_one_sample_beyond_the_top_is_refused_before_anything_is_allocated():
    """(A refusal launches nothing: the engine is never built.)"""
    for name, words in (("c1_top", "hidden activation"), ("v384", "hidden activation")):
        kw, B, _, _ = ENGINES[name]
        m = _model(kw)
        with pytest.raises(RuntimeError, match=words):
            m.reserve(B + 1)
        del m
    kw = _cfg(768, 32, 2, mult=1)
    m = _model(kw)
    with pytest.raises(RuntimeError, match="the largest max_batch that fits is 5461;"):
        m.reserve(5462)
    del m
    _free()


# ---- 2. the sampler ------------------------------------------------------------------------------------------------------------------------------------------------
# One call of the request entries may need at most 1024 conditioning rows (kMaxRequestCondRows: distinct noise levels + one label row per request + 1), so 1365
# requests -- 2730 model rows -- cannot ride in one generate_latents_requests call: that call is asked as a refusal, the top of the range is run through the uniform
# entry (generate_latents: one table for the whole batch, no such cap), and the request entry at 1000 requests (2000 model rows: hid 2.93 GiB).
def _sampler_inputs():
    g = torch.Generator().manual_seed(77)
    eps, z0 = torch.randn(P, 4, 32, 32, generator=g), torch.randn(P, 4, 32, 32, generator=g)
    lab = torch.randn(P, 768, generator=g) * 0.5
    lab[1] = 0
    return eps, z0, lab


def test_sampler_uniform_call_at_2730_model_rows_equals_three_at_a_time():
    """One CFG call of 1365 images (2730 model rows: block 0 on the shared half batch and its fan-out), n_iter 3.  Device bytes: the c1_top engine, 19.4 GiB."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    kw, B = _cfg(768, 32, 2), 1365
    need = _engine_bytes(kw, 2 * B, False)
    _need_free(need, "the sampler engine")
    t0 = time.time()
    dev = _dev()
    m = _model(kw)
    try:
        m.reserve(2 * B)
        gen = DiffusionGenerator(m, None, dev, torch.float32)
        eps, _, lab = _sampler_inputs()
        call = lambda idx: gen.generate_latents(lab[idx].to(dev), n_iter=3, num_imgs=len(idx), class_guidance=4.5, seeds=eps[idx].to(dev), sharp_f=0.1, bright_f=0.1)
        ref = call(torch.arange(P)).clone()
        assert bool(torch.isfinite(ref).all()) and not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2])
        idx = replica_map(B)
        big = call(idx)
        torch.cuda.synchronize()
        n_bad, first = mismatches(big, ref, idx.to(dev))
        again = call(torch.arange(P))
        _record(f"sampler, uniform entry: {B} images, 2 x {B} model rows of 256 tokens, n_iter 3, guidance 4.5; mismatching images {n_bad}; three afterwards equal "
                f"{bool(torch.equal(again, ref))}; {time.time() - t0:.1f} s")
        assert n_bad == 0, f"{n_bad} of {B} images differ from the image in a call of three; first {first}; last {B - 1}; at 2^31 bytes of hid: model row 1365"
        assert torch.equal(again, ref)
    finally:
        del m
        _free()


def test_sampler_requests_at_2000_model_rows_equal_the_requests_three_at_a_time():
    """One generate_latents_requests call of 1000 requests (2000 model rows, hid 2.93 GiB: the source-row table, per-request guidance), n_iter 3: one kind of request
    at guidance exactly 1, one masked image-to-image, one plain.  1365 requests in one call are refused by the conditioning-row cap before anything is enqueued.
    Device bytes: an engine of 2000 samples, 14.7 GiB."""
    from transformer_latent_diffusion_amd import DiffusionGenerator
    kw, B = _cfg(768, 32, 2), 1000
    need = _engine_bytes(kw, 2 * B, False)
    _need_free(need, "the sampler engine")
    t0 = time.time()
    dev = _dev()
    m = _model(kw)
    try:
        m.reserve(2 * B)
        gen = DiffusionGenerator(m, None, dev, torch.float32)
        eps, z0, lab = _sampler_inputs()
        mask = torch.ones(P, 1, 32, 32)
        mask[2, :, 8:24, 4:20] = 0                                        # request kind 2 keeps a rectangle of its initial latent
        guid, strength = [4.5, 1.0, 3.0], [None, None, 0.7]

        def call(idx):
            il = idx.tolist()
            return gen.generate_latents_requests(lab[idx].to(dev), seeds=eps[idx].to(dev), n_iter=3, class_guidance=[guid[r] for r in il], init_latents=z0[idx].to(dev),
                                                 strength=[strength[r] for r in il], mask=mask[idx].to(dev), sharp_f=0.1, bright_f=0.1)

        ref = call(torch.arange(P)).clone()
        assert bool(torch.isfinite(ref).all()) and not torch.equal(ref[0], ref[1]) and not torch.equal(ref[1], ref[2])
        with pytest.raises(ValueError, match="conditioning rows"):
            call(replica_map(1365))
        idx = replica_map(B)
        big = call(idx)
        torch.cuda.synchronize()
        n_bad, first = mismatches(big, ref, idx.to(dev))
        again = call(torch.arange(P))
        _record(f"sampler, request entry: {B} requests, 2 x {B} model rows of 256 tokens, n_iter 3, guidance {guid}, strength {strength}; mismatching requests {n_bad}; "
                f"three afterwards equal {bool(torch.equal(again, ref))}; {time.time() - t0:.1f} s")
        assert n_bad == 0, f"{n_bad} of {B} requests differ from the request in a call of three; first {first}; last {B - 1}; at 2^31 bytes of hid: model row 1365"
        assert torch.equal(again, ref)
    finally:
        del m
        _free()


# ---- 3. the training engine ----------------------------------------------------------------------------------------------------------------------------------------
# name: (config, max_batch).  One block.  The second is the largest max_batch the guard admits at that shape; the third has 4096 tokens: both attention-backward kernels.
TRAINERS = {
    "d768_2048": (_cfg(768, 32, 1), 2048),            # M = 524 288: 3.0 GiB per [M, hid] buffer, 2.25 GiB per [M, 3 d]
    "d768_top": (_cfg(768, 32, 1), 2714),             # T1 / T2 = (M + 4096) x 3072 x 2 B = 3.9999 GiB
    "d128_g64": (_cfg(128, 128, 1), 1022),            # M = 4 186 112 rows of 4096-token samples: T1 / T2 3.9999 GiB, the row chunks one short of the y axis
}


def _trainer_bytes(kw, B):
    g = kw["image_size"] // kw["patch_size"]
    M, d = B * g * g, kw["embed_dim"]
    hid = d * kw["mlp_multiplier"]
    wide = max(hid, 3 * d)
    per_layer = M * (13 * d * 2 + 2 * d * 2 + 3 * hid * 2 + 3 * 8 + 8 * (d // 64))
    shared = M * (4 * d * 4 + 3 * d * 2 + hid * 2 + 3 * d * 2) + 2 * (M + 4096) * wide * 2 + M * 64 * 4 * 6
    io = 6 * B * kw["n_channels"] * kw["image_size"] ** 2 * 4
    return kw["n_layers"] * per_layer + shared + io + 3 * GIB


def _trainer(kw, B, **extra):
    from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
    return Trainer(DenoiserConfig(**kw), device=_dev(), max_batch=B, init_seed=5, keep_ema=False, use_graph=False, **extra)


def _train_three(kw, seed):
    g = torch.Generator().manual_seed(seed)
    S, Cn = kw["image_size"], kw["n_channels"]
    xn, tgt = torch.randn(P, Cn, S, S, generator=g), torch.randn(P, Cn, S, S, generator=g)
    lab = torch.randn(P, 768, generator=g) * 0.5
    lab[1] = 0
    return xn, torch.tensor([0.2, 0.55, 0.9]), lab, tgt


def _backward_batch(B):
    """(batch, active samples) of the sparse backward: the largest batch <= B that is a power of two times its number of active samples (at least four) -- the
    loss scale 1 / numel of the large call is then the reference's times an exact power of two, which bf16 and fp32 roundings commute with."""
    for p2 in (512, 256, 128, 64):
        if B // p2 >= 4:
            return (B // p2) * p2, B // p2
    raise AssertionError(B)


def _active_samples(kw, Bb, n_act):
    """Sample 0, the last, the two that straddle 2^31 bytes of the [M, hid] and the [M, 3 d] buffers, and others spread between them -- no two adjacent."""
    g = kw["image_size"] // kw["patch_size"]
    N, d = g * g, kw["embed_dim"]
    s_hid, s_dqkv = (1 << 31) // (N * d * kw["mlp_multiplier"] * 2), (1 << 31) // (N * 3 * d * 2)
    assert 0 < s_hid < Bb - 1 and 0 < s_dqkv < Bb - 1
    act = [0, s_hid, s_dqkv if abs(s_dqkv - s_hid) >= 2 else s_hid + 2, Bb - 1]
    k = 1
    while len(act) < n_act:
        c = (k * 2654435761 >> 5) % Bb
        k += 1
        if all(abs(c - a) >= 2 for a in act):
            act.append(c)
    act = sorted(act)
    assert len(act) == n_act and all(b - a >= 2 for a, b in zip(act, act[1:])) and act[-1] == Bb - 1
    return act


def trainer_checks(name, tn_arm=False):
    """The three checks of one training engine, in this process; returns the record (a dict of figures).  Raises AssertionError on a failure."""
    kw, B = TRAINERS[name]
    t0 = time.time()
    dev = _dev()
    tr = _trainer(kw, B, skip_nonfinite=True)
    out = {"name": name, "max_batch": B, "tn_wgrad": os.environ.get("TLD_TRAIN_TN_WGRAD", "1")}
    try:
        xn, nl, lab, tgt = (t.to(dev) for t in _train_three(kw, 300 + len(name)))
        idx = replica_map(B).to(dev)
        # forward: sample_loss and pred of every sample against the sample in a batch of three
        _, s3, p3 = tr.forward_loss(xn, nl, lab, tgt)
        s3, p3 = s3.clone(), p3.clone()
        assert bool(torch.isfinite(p3).all()) and not torch.equal(p3[0], p3[1])
        big_xn, big_nl, big_lab = xn[idx], nl[idx], lab[idx]
        _, sB, pB = tr.forward_loss(big_xn, big_nl, big_lab, tgt[idx])
        torch.cuda.synchronize()
        bad_p, first_p = mismatches(pB, p3, idx)
        bad_s, first_s = mismatches(sB.view(-1, 1), s3.view(-1, 1), idx)
        out.update(pred_mismatches=bad_p, sample_loss_mismatches=bad_s)
        Bb, n_act = _backward_batch(B)
        act = _active_samples(kw, Bb, n_act)
        assert bad_p == 0 and bad_s == 0, f"{name}: pred of {bad_p} (first {first_p}) and sample_loss of {bad_s} (first {first_s}) samples differ; active / straddling samples {act}"
        if tn_arm and name != "d768_2048":
            return out
        # backward, made local: target = pred except on the four active samples
        a = torch.tensor(act, device=dev)
        target = pB[:Bb].clone()
        target[a] = tgt[idx[a]]
        del pB
        big_xn, big_nl, big_lab = big_xn[:Bb], big_nl[:Bb], big_lab[:Bb]
        loss_big, _ = tr.forward_backward(big_xn, big_nl, big_lab, target)
        g_big, loss_big = tr.grads.clone(), float(loss_big)
        sl = tr.sample_loss()
        inactive = torch.ones(Bb, dtype=torch.bool, device=dev)
        inactive[a] = False
        assert bool((sl[inactive] == 0.0).all()), f"{name}: {int((sl[inactive] != 0).sum())} inactive samples have a loss that is not exactly 0.0"
        assert bool((sl[a] > 0).all())
        loss_4, _ = tr.forward_backward(big_xn[a], big_nl[a], big_lab[a], target[a])
        g_4, loss_4 = tr.grads.clone(), float(loss_4)
        scale = float(Bb // n_act)
        worst, worst_key, ratios = 0.0, "", {}
        for key, (off, shape) in tr.layout.items():
            n = int(np.prod(shape))
            x, y = g_big[off:off + n].double() * scale, g_4[off:off + n].double()
            ref_max = float(y.abs().max())
            assert ref_max > 0 and bool(torch.isfinite(x).all()), key
            r = float((x - y).abs().max()) / ref_max
            ratios[key] = r
            if r > worst:
                worst, worst_key = r, key
        rl = abs(loss_big * scale - loss_4) / abs(loss_4)
        out.update(backward_batch=Bb, active=act, grad_worst_ratio=worst / EXACT, grad_worst_tensor=worst_key, loss_ratio=rl / EXACT, tensors=len(ratios))
        over = {k: v / EXACT for k, v in ratios.items() if v > EXACT}
        assert not over, f"{name}: gradient tensors beyond the EXACT bound (ratio to it): {over}; active samples {act}"
        assert rl <= EXACT, (loss_big * scale, loss_4)
        if not tn_arm:
            # one training step at the full size: a smoke assertion beside the real ones
            from transformer_latent_diffusion_amd import DeviceLatentDataset
            g = torch.Generator().manual_seed(9)
            S, Cn = kw["image_size"], kw["n_channels"]
            ds = DeviceLatentDataset(torch.randn(8, Cn, S, S, generator=g), torch.randn(8, 768, generator=g) * 0.5, device=dev)
            loss = tr.train_step_from(ds, torch.arange(B, device=dev) % 8)
            st = tr.optimizer_stats()
            out.update(step_loss=float(loss), step_grad_norm=st["grad_norm"])
            assert np.isfinite(float(loss)) and np.isfinite(st["grad_norm"]) and st["applied_steps"] == 1 and st["skipped_steps"] == 0, st
        out["seconds"] = round(time.time() - t0, 1)
        return out
    finally:
        del tr
        _free()


@pytest.mark.parametrize("name", list(TRAINERS))
def test_trainer_forward_backward_and_step_at_large_batch(name):
    kw, B = TRAINERS[name]
    need = _trainer_bytes(kw, B)
    _need_free(need, f"trainer {name}")
    rec = trainer_checks(name)
    _record(f"trainer {name}: needs {need / GIB:.1f} GiB; " + json.dumps(rec))


def child_main(name, path):
    with open(path, "w") as f:
        json.dump(trainer_checks(name, tn_arm=True), f)


def test_trainer_backward_with_the_transposing_weight_gradient(tmp_path):
    """TLD_TRAIN_TN_WGRAD=0 (read at tld_train_create: a fresh child process, the only second process of this file): the weight gradients go through the transposed
    operands T1 / T2 and launch_gemm's split-K form at M = 524 288."""
    kw, B = TRAINERS["d768_2048"]
    need = _trainer_bytes(kw, B)
    _need_free(need, "trainer d768_2048 (transposing weight gradient)")
    _free()
    path = str(tmp_path / "tn_arm.json")
    code = "import sys; sys.path.insert(0, 'tests'); import test_gpu_large_offsets as T; T.child_main(sys.argv[1], sys.argv[2])"
    r = subprocess.run([sys.executable, "-c", code, "d768_2048", path], env=dict(os.environ, TLD_TRAIN_TN_WGRAD="0"), capture_output=True, text=True, cwd=REPO, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    with open(path) as f:
        rec = json.load(f)
    assert rec["tn_wgrad"] == "0" and rec["grad_worst_ratio"] <= 1.0
    _record("trainer d768_2048, TLD_TRAIN_TN_WGRAD=0 (child process): " + json.dumps(rec))


# ---- 4. the kernel hooks alone -----------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


DW_TOL = 6e-3        # tests/test_gpu_dwconv.py: rel-rms against conv + exact GELU of the same bf16 inputs


def _dwconv(x, wf, bf, batch, grid, channels):
    from transformer_latent_diffusion_amd import _lib
    out = torch.full_like(x, float("nan"))              # every element must be written
    _lib.check(_lib.lib().tld_debug_dwconv_gelu(x.data_ptr(), wf.ctypes.data_as(C.POINTER(C.c_float)), bf.ctypes.data_as(C.POINTER(C.c_float)), out.data_ptr(), batch, grid,
                                                channels, _stream()), "tld_debug_dwconv_gelu")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("grid,batch", [(16, 2730), (32, 400), (32, 682)])
def test_dwconv_hook_replicas(grid, batch):
    """3072 channels: the whole-image kernel at 3.999 GiB, the row-streaming kernel at 2.34 and 3.996 GiB (its 32-bit ooff above 2^31 and at the top).  Device bytes:
    input + output + the compare's chunks, 2 x batch x grid^2 x 3072 x 2 B + 2 GiB."""
    channels = 3072
    nbytes = batch * grid * grid * channels * 2
    _need_free(2 * nbytes + 2 * GIB, f"dwconv hook grid {grid} batch {batch}")
    t0 = time.time()
    dev = _dev()
    g = torch.Generator().manual_seed(grid + batch)
    x3 = torch.randn(P, grid * grid, channels, generator=g).to(torch.bfloat16)
    w = (torch.randn(channels, 1, 3, 3, generator=g) * 0.4).float()
    b = (torch.randn(channels, generator=g) * 0.2).float()
    wf, bf = np.ascontiguousarray(w.reshape(channels, 9).numpy()), np.ascontiguousarray(b.numpy())
    x3d = x3.to(dev)
    ref = _dwconv(x3d, wf, bf, P, grid, channels)
    # the three replicas against float64 (conv as nine shifted products, exact GELU), the bound of tests/test_gpu_dwconv.py
    img = torch.nn.functional.pad(x3d.double().view(P, grid, grid, channels), (0, 0, 1, 1, 1, 1))
    w64 = w.to(dev).double().view(channels, 3, 3)
    acc = b.to(dev).double().expand(P, grid, grid, channels).clone()
    for du in range(3):
        for dv in range(3):
            acc += img[:, du:du + grid, dv:dv + grid, :] * w64[:, du, dv]
    r64 = (0.5 * acc * (1.0 + torch.erf(acc / np.sqrt(2.0)))).view(P, grid * grid, channels)
    rel = float((ref.double() - r64).pow(2).mean().sqrt() / r64.pow(2).mean().sqrt())
    assert rel <= DW_TOL, rel
    del img, acc, r64
    idx = replica_map(batch).to(dev)
    big = _dwconv(x3d[idx], wf, bf, batch, grid, channels)
    n_bad, first = mismatches(big, ref, idx, chunk=64)
    s31 = (1 << 31) // (grid * grid * channels * 2)
    _record(f"dwconv hook grid {grid}, batch {batch}, {channels} channels: {nbytes} bytes ({nbytes / GIB:.3f} GiB); three replicas rel-rms against float64 {rel:.2e} "
            f"(bound {DW_TOL}); mismatching samples {n_bad}; {time.time() - t0:.1f} s")
    del big
    _free()
    assert n_bad == 0, f"{n_bad} of {batch} samples differ from their replica; first {first}; the sample at 2^31 bytes {s31}, the last {batch - 1}"


ATT_TOL, ATT_ROW_TOL = 5e-3, 2e-2        # tests/test_gpu_attention.py


@pytest.mark.parametrize("N,B,H", [(256, 2730, 12), (256, 5461, 12), (1024, 1024, 12)])
def test_attention_fwd_hook_replicas(N, B, H):
    """q|k [B N, 2 d] of 2.0, 4.0 and 3.0 GiB.  Device bytes: qk + vt + att + the compare's chunks, B x N x d x 2 B x 4 + 2 GiB."""
    from test_gpu_attention import _ref, _run
    d = 64 * H
    _need_free(B * N * d * 2 * 5 + 2 * GIB, f"attention hook N {N} B {B}")
    t0 = time.time()
    dev = _dev()
    g = torch.Generator().manual_seed(N + B)
    q, k, v = (torch.randn(P, N, H, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    ref = _run(P, N, H, q, k, v)
    got, want = ref.float().reshape(P, N, H, 64), _ref(q, k, v)
    r = float((got - want).pow(2).mean().sqrt() / want.pow(2).mean().sqrt())
    row = ((got - want).pow(2).sum(-1).sqrt() / want.pow(2).sum(-1).sqrt().clamp_min(1e-6)).max().item()
    assert r <= ATT_TOL and row <= ATT_ROW_TOL, (r, row)
    from transformer_latent_diffusion_amd import _lib
    idx = replica_map(B).to(dev)
    qk3 = torch.cat([q.reshape(P, N, d), k.reshape(P, N, d)], dim=2).to(dev)
    vt3 = v.permute(0, 2, 3, 1).reshape(P, d, N).contiguous().to(dev)
    qk, vt = qk3[idx].view(B * N, 2 * d), vt3[idx]
    att = torch.full((B * N, d), float("nan"), dtype=torch.bfloat16, device=dev)              # every element must be written
    _lib.check(_lib.lib().tld_debug_attention_fwd(qk.data_ptr(), vt.data_ptr(), att.data_ptr(), B, N, H, 1, None, _stream()), "tld_debug_attention_fwd")
    torch.cuda.synchronize()
    n_bad, first = mismatches(att.view(B, N, d), ref.view(P, N, d), idx)
    qk_bytes = B * N * 2 * d * 2
    _record(f"attention forward hook {N} tokens, batch {B}, {H} heads: q|k {qk_bytes} bytes ({qk_bytes / GIB:.3f} GiB); three replicas rel-rms {r:.2e}, worst row {row:.2e}; "
            f"mismatching samples {n_bad}; {time.time() - t0:.1f} s")
    del qk, vt, att
    _free()
    assert n_bad == 0, f"{n_bad} of {B} samples differ; first {first}; the sample at 2^31 bytes of q|k {(1 << 31) // (N * 2 * d * 2)}, the last {B - 1}"


def test_wgrad_hook_sparse_rows():
    """dW = dY^T X at 524 288 rows, n_out 3072 (dY 3.0 GiB), k_in 768: dY all zero except four 64-row groups -- the first, the last, and the ones holding byte 2^31 of
    dY and of an [M, 3 d]-sized prefix -- against the float64 product of those 256 rows, EXACT.  Device bytes: dY + X + slices, 3.0 + 0.75 + 0.3 GiB + 2 GiB."""
    from transformer_latent_diffusion_amd import _lib
    rows, n_out, k_in = 524288, 3072, 768
    _need_free(rows * (n_out + k_in) * 2 + 3 * GIB, "wgrad hook")
    t0 = time.time()
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(3)
    X = torch.empty(rows, k_in, dtype=torch.bfloat16, device=dev)
    for r0 in range(0, rows, 65536):
        X[r0:r0 + 65536] = torch.randn(65536, k_in, generator=g, device=dev).to(torch.bfloat16)
    dY = torch.zeros(rows, n_out, dtype=torch.bfloat16, device=dev)
    groups = sorted({0, ((1 << 31) // (n_out * 2)) // 64, ((1 << 31) // (2304 * 2)) // 64, rows // 64 - 1})
    assert len(groups) == 4
    live = torch.cat([torch.arange(64) + 64 * gr for gr in groups]).to(dev)
    dY[live] = torch.randn(256, n_out, generator=g, device=dev).to(torch.bfloat16)
    slice_floats = 32 * n_out * k_in
    slices = torch.empty(slice_floats, device=dev)
    dW = torch.full((n_out, k_in), float("nan"), device=dev)
    _lib.check(_lib.lib().tld_debug_wgrad(dY.data_ptr(), X.data_ptr(), dW.data_ptr(), slices.data_ptr(), slice_floats, rows, n_out, k_in, _stream()), "tld_debug_wgrad")
    torch.cuda.synchronize()
    ref = dY[live].double().T @ X[live].double()
    err = float((dW.double() - ref).abs().max() / ref.abs().max())
    _record(f"wgrad hook rows {rows}, n_out {n_out}, k_in {k_in}: live 64-row groups {groups}; max |d| / max |ref| {err:.3e} = {err / EXACT:.3f} of the EXACT bound; {time.time() - t0:.1f} s")
    del dY, X, slices
    _free()
    assert err <= EXACT, (err, groups)


@pytest.mark.parametrize("N,B", [(256, 2730), (1024, 700)])
def test_attention_bwd_hook_replicas(N, B):
    """dqkv [B N, 3 d] bf16 of 3.0 and 3.1 GiB, 12 heads: the single-workgroup kernel (256 tokens) and the two-kernel form (1024).  Three replicas against the float64
    model of tests/test_gpu_attn_bwd_classes.py, every sample of the large call against its replica.  Device bytes: qk, vt, o, g (fp32), dqkv and scratch:
    B x N x 768 x 22 B + 2 GiB."""
    import test_gpu_attn_bwd_classes as A
    from transformer_latent_diffusion_amd import _lib
    H = 12
    d = 64 * H
    _need_free(B * N * d * 22 + 2 * GIB, f"attention backward hook N {N} B {B}")
    t0 = time.time()
    dev = _dev()
    gen = torch.Generator().manual_seed(5000 + N)
    rn = lambda *sh: torch.randn(*sh, generator=gen)
    q, k, v, g = A._bf(rn(P, N, d) * 1.5), A._bf(rn(P, N, d)), A._bf(rn(P, N, d)), rn(P, N, d) * 0.1
    o, exact, model = A.references(q, k, v, g, H)
    ref = A.launch(q, k, v, o, g, H)                                     # [3 N, 3 d] bf16, sentinels checked
    nw = 8 if N % 256 == 0 else A.dispatch(N)[1]
    fail = A.compare(f"large offsets N={N} three replicas", ref.double(), exact, model, H, nw, N)
    assert not fail, fail
    idx = replica_map(B).to(dev)
    qk3 = torch.cat([q, k], dim=-1).bfloat16().to(dev)
    vt3 = v.view(P, N, H, 64).permute(0, 2, 3, 1).contiguous().bfloat16().to(dev)
    qk, vt, ob, gd = qk3[idx], vt3[idx], o.to(dev)[idx], g.to(dev)[idx]
    out = torch.full((B * N, 3 * d), float("nan"), dtype=torch.bfloat16, device=dev)
    scratch = torch.zeros(2 * B * H * N, device=dev)
    p_ = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().tld_debug_attention_bwd(p_(qk), p_(vt), p_(ob), p_(gd), p_(out), p_(scratch), B, N, H, _stream()), "tld_debug_attention_bwd")
    torch.cuda.synchronize()
    n_bad, first = mismatches(out.view(B, N, 3 * d), ref.view(P, N, 3 * d), idx)
    nbytes = B * N * 3 * d * 2
    _record(f"attention backward hook {N} tokens, batch {B}, {H} heads: dqkv {nbytes} bytes ({nbytes / GIB:.3f} GiB); three replicas inside the class bounds; "
            f"mismatching samples {n_bad}; {time.time() - t0:.1f} s")
    del qk, vt, ob, gd, out, scratch
    _free()
    assert n_bad == 0, f"{n_bad} of {B} samples differ; first {first}; the sample at 2^31 bytes of dqkv {(1 << 31) // (N * 3 * d * 2)}, the last {B - 1}"


# ---- the GEMM epilogues with an output beyond 2 GiB: all rows of A zero except four 256-row tiles -- the first, the last, and the ones holding byte 2^31 of the
# ---- output and of the A operand (or the middle).  Zero rows must come out as the bias path alone gives them, exactly; the live tiles are held per element
# ---- against float64 by the bound of tests/test_gpu_gemm_epilogues.py (its reference() on the live rows).
# name: (epilogue, M, N, K, extras, bytes per output row)
GEMM_BIG = {
    "bias": (2, 524288, 3072, 768, {}, 3072 * 2),                           # bias -> bf16: 3.0 GiB (the up-projection at M = 524 288)
    "qkv": (1, 699136, 2304, 768, {"ntok": 256}, 1536 * 2),                  # q | k 2.0002 GiB + the V^T image of 2731 samples
    "resid_stats": (3, 1400064, 768, 64, {"stats": 1}, 768 * 2),             # residual add in place, 2.003 GiB, + the LayerNorm-1 partial sums
    "fp32": (0, 262144, 3072, 64, {}, 3072 * 4),                              # fp32 C: 3.0 GiB
}


def _live_rows(M, row_bytes, a_row_bytes):
    nt = M // 256
    tiles = {0, min(((1 << 31) // row_bytes) // 256, nt - 1), min(((1 << 31) // a_row_bytes) // 256, nt // 2), nt - 1}
    for extra in (nt // 3, nt // 5):
        if len(tiles) < 4:
            tiles.add(extra)
    tiles = sorted(tiles)
    assert len(tiles) == 4 and tiles[-1] == nt - 1
    return tiles, torch.cat([torch.arange(256) + 256 * t for t in tiles])


@pytest.mark.parametrize("name", list(GEMM_BIG))
def test_gemm_epilogue_hook_output_beyond_2_gib(name):
    """Device bytes: A + the output(s) + the compare's chunks: at most 2 x the output + 3 GiB."""
    import test_gpu_gemm_epilogues as E
    from transformer_latent_diffusion_amd import _lib
    epi, M, N, K, ex, row_bytes = GEMM_BIG[name]
    out_bytes = M * row_bytes
    assert out_bytes > 1 << 31
    _need_free(2 * out_bytes + 3 * GIB, f"GEMM epilogue {name}")
    t0 = time.time()
    dev = _dev()
    tiles, live = _live_rows(M, row_bytes, K * 2)
    live = live.to(dev)
    n_live = live.numel()
    c_live = (epi if epi else 1, "bf16", n_live, N, K, ex)                 # (fp32: the plain product, which reference() gives for the QKV epilogue)
    I = E.make_inputs((epi if epi else 2, "bf16", n_live, N, K, ex), dev)  # operands of the live rows, seeded by the shape
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    A[live] = I["A"]
    a = _lib.TldGemmEpilogueArgs()
    a.A, a.W, a.M, a.N, a.K, a.lda, a.ldw, a.epilogue = A.data_ptr(), I["W"].data_ptr(), M, N, K, K, K, epi
    keep = []
    if epi == 2:
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=dev)
        a.bias, a.out_bf16, a.ldo = I["bias"].data_ptr(), out.data_ptr(), N
        zero_row = I["bias"].to(torch.bfloat16)
    elif epi == 1:
        dm, ntok = N // 3, ex["ntok"]
        out = torch.full((M, 2 * dm), float("nan"), dtype=torch.bfloat16, device=dev)
        vt = torch.full((M // ntok, dm, ntok), float("nan"), dtype=torch.bfloat16, device=dev)
        a.out_bf16, a.ldo, a.vt, a.ntok, a.d = out.data_ptr(), 2 * dm, vt.data_ptr(), ntok, dm
        zero_row = torch.zeros(2 * dm, dtype=torch.bfloat16, device=dev)
    elif epi == 3:
        base = (torch.randn(N, generator=torch.Generator().manual_seed(11)) * 2).to(torch.bfloat16).to(dev)      # the residual stream of the zero rows: one row, repeated
        out = base.repeat(M, 1)
        out[live] = I["resid0"]
        stats = torch.full((M, 8, 2), float("nan"), device=dev)
        a.bias, a.resid, a.ldr, a.stats_out = I["bias"].data_ptr(), out.data_ptr(), N, stats.data_ptr()
        zero_row = (base.float() + I["bias"]).to(torch.bfloat16)            # x + (0 + bias) in fp32, rounded once
    else:
        out = torch.full((M, N), float("nan"), device=dev)
        a.c_f32, a.ldc = out.data_ptr(), N
        zero_row = torch.zeros(N, device=dev)
    _lib.check(_lib.lib().tld_debug_gemm_epilogue(C.byref(a), _stream()), f"tld_debug_gemm_epilogue({name})")
    torch.cuda.synchronize()
    # the zero rows: exactly the bias path
    is_live = torch.zeros(M, dtype=torch.bool, device=dev)
    is_live[live] = True
    n_bad, first = 0, []
    for s0 in range(0, M, 65536):
        e0 = min(s0 + 65536, M)
        bad = ((_bits(out[s0:e0]) != _bits(zero_row)[None, :]).any(1) & ~is_live[s0:e0]).nonzero().flatten()
        n_bad += int(bad.numel())
        first += (bad[:4] + s0).tolist()
    # the live tiles: per element against float64
    ref, bound = E.reference(c_live, I)
    if epi == 0:
        bound = bound - 2.0 ** -8 * ref.abs()                              # fp32 output: no rounding to bf16, the accumulation term alone
    got = out[live]
    if epi == 1:
        dm, ntok = N // 3, ex["ntok"]
        worst = float(((got.double() - ref[:, :2 * dm]).abs() / bound[:, :2 * dm]).max())
        samples = torch.unique(live // ntok)
        v_got = vt[samples].permute(0, 2, 1).reshape(-1, dm)                # [live rows][feature]: 256-row tiles are whole samples here
        worst = max(worst, float(((v_got.double() - ref[:, 2 * dm:]).abs() / bound[:, 2 * dm:]).max()))
        dead = torch.ones(M // ntok, dtype=torch.bool, device=dev)
        dead[samples] = False
        n_bad += int((_bits(vt[dead]) != 0).any(-1).any(-1).sum())
    else:
        worst = float(((got.double() - ref).abs() / bound).max())
    if epi == 3:      # the partial sums of the STORED values, every row: 96 fp32 additions per slot (the bound of tests/test_gpu_gemm_epilogues.py)
        nslot = N // 96
        for s0 in range(0, M, 131072):
            x = out[s0:s0 + 131072].double().view(-1, nslot, 96)
            st = stats[s0:s0 + 131072, :nslot].double()
            for j, (want, mag) in enumerate(((x.sum(2), x.abs().sum(2)), ((x * x).sum(2), (x * x).sum(2)))):
                worst = max(worst, float(((st[:, :, j] - want).abs() / (97 * 2.0 ** -24 * mag + 1e-30)).nan_to_num(nan=float("inf")).max()))
    _record(f"GEMM epilogue hook {name}: M {M}, N {N}, K {K}: output {out_bytes} bytes ({out_bytes / GIB:.3f} GiB); live 256-row tiles {tiles}; zero rows that differ from the "
            f"bias path {n_bad}; live tiles (and statistics) max error / bound {worst:.3f}; {time.time() - t0:.1f} s")
    del A, out
    _free()
    assert n_bad == 0, f"{name}: {n_bad} zero rows differ from the bias path alone; first {first[:8]}; live tiles {tiles}"
    assert worst <= 1.0, (name, worst)


def test_gemm_splitk_hook_slices_beyond_2_gib():
    """tld_debug_gemm_splitk, four K-splits at M = 262 144, N = 768, K = 256: fp32 slices [4][M][768] of 3.0 GiB; A zero except four 256-row tiles.  Device bytes: 3.2 + 2 GiB."""
    from transformer_latent_diffusion_amd import _lib
    M, N, K, ks = 262144, 768, 256, 4
    _need_free(ks * M * N * 4 + 3 * GIB, "split-K hook")
    t0 = time.time()
    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(21)
    tiles, live = _live_rows(M, 12288, K * 2)      # byte 2^31 of the slices lies in slice 2 at row 174 762 = tile 682, which is (2^31 / (4 N x 4 B)) / 256
    live = live.to(dev)
    A = torch.zeros(M, K, dtype=torch.bfloat16, device=dev)
    A[live] = torch.randn(live.numel(), K, generator=g, device=dev).to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g, device=dev) * 0.1).to(torch.bfloat16)
    slices = torch.full((ks, M, N), float("nan"), device=dev)
    _lib.check(_lib.lib().tld_debug_gemm_splitk(A.data_ptr(), W.data_ptr(), slices.data_ptr(), M, N, K, ks, _stream()), "tld_debug_gemm_splitk")
    torch.cuda.synchronize()
    is_live = torch.zeros(M, dtype=torch.bool, device=dev)
    is_live[live] = True
    n_bad = sum(int(((_bits(slices[k_]) != 0).any(1) & ~is_live).sum()) for k_ in range(ks))
    kk = K // ks
    ref = torch.stack([A[live][:, k_ * kk:(k_ + 1) * kk].double() @ W[:, k_ * kk:(k_ + 1) * kk].double().T for k_ in range(ks)])
    err = float((slices[:, live].double() - ref).abs().max() / ref.abs().max())
    _record(f"split-K hook M {M}, N {N}, K {K}, {ks} splits: slices {ks * M * N * 4} bytes ({ks * M * N * 4 / GIB:.3f} GiB); live tiles {tiles}; zero rows not zero {n_bad}; "
            f"max |d| / max |ref| {err:.3e} = {err / EXACT:.3f} of the EXACT bound; {time.time() - t0:.1f} s")
    del A, slices
    _free()
    assert n_bad == 0 and err <= EXACT, (n_bad, err)

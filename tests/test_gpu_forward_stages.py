"""GPU: the denoiser's inference forward and the sampler's steps, stage by stage against float64, every block, on the engine's own inputs.

tld_engine_set_debug poisons the engine's buffers with NaN, keeps every stage of every block of one forward (or of one sampler step, CFG
layer-0 sharing on) and records the launch path of every size-dependent dispatch.  Each transition is recomputed in float64
(tests/infer_stage_refs.py, held against the reference fixtures on the host by tests/test_infer_stage_refs_host.py) from the engine's
snapshot of its inputs and the operands as the engine holds them (blk<i>.wqkv ..., the folds' c1 / b1 vectors, the conditioning tables), and
compared with the engine's snapshot of its output.  Errors do not pile up, so the bounds are per element, or per class where a kernel rounds
inside.  The constants are the project's own (tests/test_gpu_train_stages.py, tests/test_gpu_gemm_epilogues.py):

* EXACT (fp32 results where only the summation order differs: the conditioning rows and tables, each from the engine's previous row, row
  statistics and partial sums, x + att, the split-K slices, the tail output, CFG / update / start_mix): |got - ref| <= 2e-5 max|ref| per
  element.  The sinusoid features alone carry the rounding of their fp32 argument: 2^-23 |sigma speed| + 2e-6, as in
  tests/test_gpu_train_stages.py.
* ROUND (a float64-exact result rounded once to bf16: GEMM outputs including the LayerNorm folds, residual adds, LayerNorm outputs, tokens0,
  cross_row's new residual row, the whole-image depthwise + GELU, the split-K finisher):
  |got - ref| <= 2^-8 |ref| + 2e-5 sqrt(max(K, 64) / 64) max|ref|.  Without the LayerNorm-3 fold cross_row normalises the fp32 row it holds, not
  the rounded row it stores: xn3 is held against LN3 of the float64 row.
  Statistics slots are compared with the sums of the rows as stored (rounded), which is what the kernels document.
* MODELLED (roundings inside the kernel: both self-attention forms, the halved-table GELU of the tiled / streaming depthwise kernels, the fused
  up-projection + depthwise epilogues with the seam kernel): no constant.  The stage is computed twice in float64 -- exactly, and with the
  roundings the kernels document (infer_stage_refs.attn_model, dw_gelu_model; fused forms: q | k | v or the pre-activation rounded to bf16
  first; the stored result rounded to bf16 last).  The relative rms between the two is the yardstick, the bound is twice it, over the whole
  tensor and member by member of every class (where a model's error is near zero the ROUND bound holds instead): first / last row, last partial 256-row tile, sample, (sample, head), corner / edge / interior / tile-seam pixels,
  cross_row workgroup boundaries, the unconditional half and the all-zero label row.

Every compared tensor is first checked for NaN / Inf (the poison), with the count in the message.  CASES together reach every launch path:
test_cases_reach_every_launch_path holds the union of tld_engine_debug_paths against the full mask.  With TLD_FORWARD_STAGE_RECORD=<file>
a summary per case is appended to that file -- per tolerance class the worst comparison, per MODELLED transition every class's yardstick and
measured value (the worst over the blocks); stdout carries every comparison: profiles/r11_forward_stage_errors.txt is such a run.

Found by this file: dwconv_gelu_tiled_kernel (token grids wider than 16 that are not a multiple of 32: 24, 40 ...) took the clamped copy in its
halo for the zero padding right of the image when the last tile is partial.  Cases V192 (grid 24) and V320 (grid 40): last row 7.4e-1, corner
5.2e-1, edge 3.7e-1, whole tensor 9.6e-2 ... 1.3e-1 against bounds of 3.4e-3.  Fixed in the kernel; grids that are multiples of 16 compute the
same bits.

On an MI355X the measured error of every MODELLED transition equals its yardstick to three digits (self-attention 1.7e-3 ... 2.3e-3, fused
up-projection + depthwise 3.0e-3 ... 3.3e-3, halved-table GELU 1.7e-3); the worst ROUND comparison is 0.99 of its bound, the worst EXACT one
3.0e-6 against 2e-5.

The checks bite (profiles/r11_forward_stage_mutations.txt).
Eight numeric, in-bounds mutations of the kernels, one library each (selected with TLD_LIB), each run once on an MI355X: this file (34 tests), then the older
forward tests of tests/test_gpu_parity.py (test_g1_stages_tiny32, test_forward_vs_golden, the 25-shape sweep, the g2 / g5 trajectories: "old", 34 tests).
  1 cross_row_mfma_kernel, LN3 rstd of the last row of each 16-row group scaled by 1 + 1 / (2 (d - 1)) when gpw > 1: 9 fail (C1, C1b, C3, C3u, C4, the four C1s
    sampler runs); LN3 rstd, EXACT: 6.2e-4 ... 6.5e-4 against 2e-5.  Old: 2 of the sweep fail (n1024_d256, n576_d768), 32 pass
  2 the x_in fan-out, label row of the unconditional half taken from the conditional half: 10 fail (every sampler run, tiny and C1s); block 0's ca, ROUND:
    8.6e+3 ... 3.3e+4 of the bound.  Old: the g2 and g5 trajectories fail (3), the forwards pass
  3 LN1 fold at blocks >= 1, the last two slots not summed (the kernel takes an even count): 13 fail; QKV q | k, ROUND, 6.1e+2 of the bound; fused QKV +
    attention, MODELLED, 1.3e-1 against 3.6e-3.  Old: 8 fail (every d = 768 forward with more than one block)
  4 splitk_resid_kernel, statistics from the unrounded row: 1 fails (LL1); LN1 partial sums, EXACT: 1.1e-3 against 2e-5.  Old: all pass
  5 dwconv_seam_kernel, the left tap of the lowest window row dropped on the lower seam row: 1 fails (C3); fused up-projection + depthwise, MODELLED, every
    class: 7.1e-2 (zero-label sample) ... 1.3e-1 (tile seam) against 6.1e-3.  Old: all pass
  6 embed_mfma_kernel, the low half of the split-bf16 weight dropped: 18 fail (every case with 16 patch features and d % 256 == 0); tokens0, ROUND: 37 ... 57
    of the bound.  Old: all pass
  7 tail_mfma_kernel, bias skipped for the last patch feature: 29 fail (every case but the plain-tail widths 192 / 320); out, EXACT: 1.2e-4 (P3) ... 6.8e-3
    (V384) against 2e-5.  Old: all pass
  8 the first update run with the second step's c1, c2 (c2 alone, as a mutation of the first step, changes nothing: x0_prev is zero there): 5 fail (every
    DPM sampler run); x_next and the trace update of step 0, EXACT: 8.1e-2 ... 1.5e-1 against 2e-5.  Old: g2 dpm fails, 33 pass
Every mutation fails here; 4, 5, 6 and 7 pass every older forward test.  The smallest margin of a MODELLED bound below the mutation that targets its
transition is 12 x (mutation 5, zero-label sample); of an EXACT bound 6 x (mutation 7, P3), of a ROUND bound 37 x (mutation 6).

Wall time on an MI355X: 42 s for this file run alone (34 tests; the four 12-block sampler cases and C1 at batch 128 take most of it).
"""
import gc
import math
import os
import re
from dataclasses import asdict

import numpy as np
import pytest
import torch

import infer_stage_refs as F
import train_stage_refs as R
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAIL_TOL = 2e-5           # EXACT: max |got - ref| / max|ref|
ROUND_C = 2e-5            # ROUND: |got - ref| <= 2^-8 |ref| + ROUND_C sqrt(max(K, 64) / 64) max|ref|
MODEL_FACTOR = 2.0        # MODELLED: measured relative rms <= MODEL_FACTOR x the rounding model's own


def _cfg(d, image, blocks, patch=2, C=4, mult=4):
    return dict(image_size=image, noise_embed_dims=256, patch_size=patch, embed_dim=d, dropout=0, n_layers=blocks, text_emb_size=768, n_channels=C,
                mlp_multiplier=mult)


# name: (config, batches run on one engine, max_batch, environment at tld_engine_create, low-latency class)
CASES = {
    "C1": (_cfg(768, 32, 12), (128,), 128, {}, 0),                       # the 100M model at the bench batch, every block: fused QKV + attention, gpw 8, fused 16 x 16 up
    "C1b": (_cfg(768, 32, 2), (37,), 128, {}, 0),                        # batch < max_batch strides, a partial last 256-row tile of cross_row's partition
    "C3": (_cfg(768, 64, 2), (16,), 16, {}, 0),                          # grid 32: LayerNorm-1 fold + chunked attention, gpw 4, fused 32 x 32 up + seam kernel
    "C3u": (_cfg(768, 64, 2), (16,), 16, {"TLD_FUSE_DWCONV": "0"}, 0),   # up-projection alone + streaming depthwise
    "C4": (_cfg(768, 128, 2), (8,), 8, {}, 0),                           # grid 64, 4096 tokens
    "W256": (_cfg(256, 32, 2), (3,), 3, {}, 0),                          # embed_mfma<2>, cross_row_mfma<1>, layernorm q4<1>, plain QKV
    "W512": (_cfg(512, 32, 2), (3,), 3, {}, 0),                          # embed_mfma<4>, cross_row_mfma<2>, layernorm q4<2>
    "P4": (_cfg(512, 64, 1, patch=4), (2,), 2, {}, 0),                   # patch 4: 64 patch features, plain embed, tail_mfma<4>
    "W1024": (_cfg(1024, 32, 2), (3,), 3, {}, 0),                        # embed_mfma<8>, cross_row_mfma<4> without LN3 statistics (xn3)
    "V192": (_cfg(192, 48, 2), (3,), 3, {}, 0),                          # VALU cross_row, generic LN, plain embed / tail; grid 24: masked attention, tiled depthwise
    "V320": (_cfg(320, 80, 2, C=8), (2,), 2, {}, 0),                     # grid 40, 8 channels
    "V384": (_cfg(384, 16, 2, patch=1, C=8, mult=2), (5,), 5, {}, 0),    # patch 1, mlp_multiplier 2
    "P3": (_cfg(768, 64, 2, patch=4, C=3), (2,), 2, {}, 0),              # 48 patch features: tail_mfma<3>
    "P2": (_cfg(256, 32, 2, C=8), (2,), 2, {}, 0),                       # 32 patch features: tail_mfma<2>
    "LL1": (_cfg(768, 32, 2), (1, 2, 8), 8, {}, 1),                      # low-latency class 1: split-K x 4, finisher <12>, the 4-wave forms
    "LL2": (_cfg(384, 16, 2), (1, 2, 8), 16, {}, 2),                     # class 2 at 64 tokens: split-K x 8, finisher <6>, whole-image depthwise, attention 64
    "F1": (_cfg(768, 32, 2), (4,), 4, {"TLD_FOLD_LN1": "0"}, 0),         # LayerNorm-1 kernel q4<3> + plain QKV + attention 256
    "F3": (_cfg(768, 32, 2), (4,), 4, {"TLD_FOLD_LN3": "0"}, 0),         # cross_row writes LN3(x)
    "FQ": (_cfg(768, 32, 2), (24,), 24, {"TLD_FUSE_QKV_ATTN": "0"}, 0),  # QKV with the LayerNorm-1 fold + attention 256; 6144 rows: the 4-wave down projection on 128-row tiles
}
IO_CASE = "W256"
FP8_PATH_CASE = (_cfg(256, 128, 1), 1)        # reaches the fp8 mode's LayerNorm kernel for the launch-path record only: the fp8 mode is held stage by stage by tests/test_gpu_fp8_stages.py


def _model(kw, seed=31):
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig
    from transformer_latent_diffusion_amd.weights import synth_state_dict
    cfg = DenoiserConfig(**kw)
    m = Denoiser(**asdict(cfg)).to(_dev())
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, seed).items()})
    return m


def _record(line):
    path = os.environ.get("TLD_FORWARD_STAGE_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Checks:
    """Comparisons of one run: rows of (transition, kind, value, bound), failures as text."""

    def __init__(self, name, B, N, G, H, gpw=1, uncond_from=None, zero_label=()):
        self.name, self.B, self.N, self.G, self.H, self.gpw = name, B, N, G, H, gpw
        self.uncond_from, self.zero_label = uncond_from, tuple(zero_label)
        self.rows, self.fail = [], []

    def _finite(self, what, got):
        bad = int((~torch.isfinite(got)).sum())
        if bad:
            self.fail.append(f"{self.name} {what}: {bad} of {got.numel()} values are NaN / Inf")
            self.rows.append((what, "finite", float("inf"), 0.0))
        return bad == 0

    def _note(self, what, kind, val, bound):
        self.rows.append((what, kind, val, bound))
        if not val <= bound:
            self.fail.append(f"{self.name} {what} [{kind}]: {val:.3e} > {bound:.3e}")

    def exact(self, what, got, ref):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if self._finite(what, got):
            self._note(what, "exact", float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)), TAIL_TOL)

    def round(self, what, got, ref, K=64):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if self._finite(what, got):
            bound = 2.0 ** -8 * ref.abs() + ROUND_C * math.sqrt(max(K, 64) / 64) * ref.abs().max()
            self._note(what, "round", float(((got - ref).abs() / bound).max()), 1.0)

    def equal(self, what, got, ref):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if self._finite(what, got):
            self._note(what, "equal", float((got != ref).sum()), 0.0)

    def classes(self, got, ref, samples, heads, pixels):
        """Relative rms of every member of every class of a [samples * N, F] tensor against ref: {class: tensor over its members}."""
        N, G, H = self.N, self.G, self.H
        e2, r2 = (got - ref) ** 2, ref ** 2
        F_ = e2.shape[-1]
        whole = float(r2.sum())
        out = {}

        def add(tag, es, rs):
            es, rs = es.reshape(-1), rs.reshape(-1)
            ok = rs > 1e-6 * whole / max(rs.numel(), 1)          # a class whose reference is (numerically) zero is held to the whole tensor's size
            rel = torch.where(ok, es / rs.clamp_min(1e-300), es / (whole / max(rs.numel(), 1)))
            out[tag] = rel.sqrt()
        add("whole", e2.sum(), r2.sum())
        rows = e2.shape[0]
        add("first row", e2[0].sum(), r2[0].sum()); add("last row", e2[-1].sum(), r2[-1].sum())
        if rows % 256:
            add("last partial tile", e2[rows - rows % 256:].sum(), r2[rows - rows % 256:].sum())
        e3, r3 = e2.view(samples, N, F_), r2.view(samples, N, F_)
        add("sample", e3.sum((1, 2)), r3.sum((1, 2)))
        if self.uncond_from is not None and samples > self.uncond_from:
            add("uncond half", e3[self.uncond_from:].sum(), r3[self.uncond_from:].sum())
        zl = [b for b in self.zero_label if b < samples]
        if zl:
            add("zero-label sample", e3[zl].sum(), r3[zl].sum())
        rw = 16 * self.gpw                                        # cross_row's partition: a workgroup walks gpw 16-row groups of one sample
        tok = torch.arange(N, device=e2.device)
        bnd = (tok % rw == 0) | (tok % rw == rw - 1)
        add("workgroup boundary rows", e3[:, bnd].sum(), r3[:, bnd].sum())
        if pixels:
            yy, xx = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
            ey, ex = (yy == 0) | (yy == G - 1), (xx == 0) | (xx == G - 1)
            masks = {"corner": ey & ex, "edge": ey ^ ex, "interior": ~(ey | ex)}
            if G > 16:       # a 256-row GEMM tile is 8 image rows at 32 x 32 (the seam kernel's rows); the depthwise kernels work on 16 x 16 tiles / 32-column strips
                masks["tile seam"] = (yy % 8 == 7) | (yy % 8 == 0) | (xx % 16 == 15) | (xx % 16 == 0)
            for tag, m in masks.items():
                m = m.reshape(-1).to(e2.device)
                add(tag, e3[:, m].sum(), r3[:, m].sum())
        if heads:
            add("(sample, head)", e3.view(samples, N, H, F_ // H).sum((1, 3)), r3.view(samples, N, H, F_ // H).sum((1, 3)))
        return out

    def modelled(self, what, got, exact, model, samples, heads=False, pixels=False, K=64):
        """got against the exact float64 result, bounded member by member of every class (each sample, each (sample, head) ...) by MODEL_FACTOR x
        the error of the rounding model against the same; the row of a class is its member with the largest measured / yardstick.  A model whose
        error over the whole tensor is below 2^-11 -- half of what one bf16 rounding of the result gives -- says nothing: ROUND then."""
        assert got.shape == exact.shape == model.shape, (what, got.shape, exact.shape, model.shape)
        if not self._finite(what, got):
            return
        yard = self.classes(model, exact, samples, heads, pixels)
        if float(yard["whole"].max()) < 2.0 ** -11:
            return self.round(what + " (model error near zero)", got, exact, K)
        meas = self.classes(got, exact, samples, heads, pixels)
        for tag in yard:
            i = int((meas[tag] / yard[tag].clamp_min(1e-300)).argmax())
            self._note(f"{what} ({tag})", f"model yardstick {float(yard[tag][i]):.3e}", float(meas[tag][i]), MODEL_FACTOR * float(yard[tag][i]))


def report(c, start=0):
    """Every comparison goes to stdout; the record file gets the case's summary: per tolerance class the number of comparisons and the worst one,
    and per MODELLED transition one line with every class's yardstick / measured pair, each the worst over the blocks."""
    rows = c.rows[start:]
    for what, kind, val, bound in rows:
        print(f"case {c.name:5s} {what:58s} {kind:30s} {val:.3e}  bound {bound:.1e}")
    strip = lambda what: re.sub(r"^blk\d+[. ]", "", what)
    for cls in ("exact", "round", "derived", "equal", "finite"):
        sel = [r for r in rows if r[1] == cls]
        if sel:
            what, _, val, bound = max(sel, key=lambda r: r[2] / r[3] if r[3] else r[2])
            _record(f"case {c.name:22s} {cls:8s} {len(sel):4d} comparisons, worst {val:.3e} of bound {bound:.1e} ({what})")
    fam = {}
    for what, kind, val, bound in rows:
        if kind.startswith("model"):
            cut = what.rindex(" (")
            slot = fam.setdefault(strip(what[:cut]), {}).setdefault(what[cut + 2:-1], [0.0, 0.0])
            if val / bound >= slot[1] / slot[0] if slot[0] else True:
                slot[0], slot[1] = bound, val
    for name, tags in fam.items():
        _record(f"case {c.name:22s} modelled {name}: yardstick / measured  " + "  ".join(f"{t} {b / MODEL_FACTOR:.2e} / {v:.2e}" for t, (b, v) in tags.items()))
    assert not c.fail, "\n".join(c.fail)


# ---- one debug call and its stages ----------------------------------------------------------------------------------------------------------
class Body:
    """The stages of one body run (a forward, or the debug step of a sampler) and what the checks need to know about it."""

    def __init__(self, m, kw, tag, B, src, noise_row, label_row, zero_label=(), checks=None):
        self.m, self.kw, self.dev = m, kw, _dev()
        self.d, self.L, self.patch, self.C = kw["embed_dim"], kw["n_layers"], kw["patch_size"], kw["n_channels"]
        self.H, self.G = self.d // 64, kw["image_size"] // kw["patch_size"]
        self.N, self.hid = self.G * self.G, self.d * kw["mlp_multiplier"]
        self.B, self.src = B, src                                  # model samples; samples up to block 0's attention (B, or B / 2 under layer-0 sharing)
        self.nrow, self.lrow = noise_row.to(self.dev), label_row.to(self.dev)
        self.paths = m.debug_paths()
        cus = torch.cuda.get_device_properties(self.dev).multi_processor_count
        gpw, gps = 1, self.N // 16
        while gpw < 16 and gps % (gpw * 2) == 0 and B * (gps // (gpw * 2)) >= cus:      # launch_cross_row's partition, CU count from the device
            gpw *= 2
        self.gpw = gpw if self.d % 256 == 0 else 1
        self.c = (checks or Checks)(tag, B, self.N, self.G, self.H, self.gpw, uncond_from=src if src < B else None, zero_label=zero_label)      # checks: a subclass with further classes
        self.w = {k: v.to(self.dev).double() for k, v in m.state_dict().items() if v.dtype != torch.int64}

    def has(self, name):
        try:
            self.m.stage_shape(name)
            return True
        except RuntimeError:
            return False

    def S(self, name):
        return torch.from_numpy(self.m.read_stage(name)).to(self.dev).double()


def check_cond(b, sigma_rows, label_rows):
    """Conditioning rows and per-layer tables: sigma_rows [Tn] and label_rows [Tl, text] are the inputs of the token rows in the engine's order."""
    c, w = b.c, b.w
    sig = sigma_rows.double().reshape(-1)
    sinb, ref = b.S("cond.sin"), F.cond_sin(w, sig)
    if c._finite("cond.sin", sinb):    # the fp32 product sigma * speed is rounded before sinf: 2^-24 |a| on the argument, + sinf's own 1e-6 (as tests/test_gpu_train_stages.py)
        c._note("cond.sin", "derived", float((sinb - ref).abs().max()), 2.0 ** -23 * float((sig.view(-1, 1) * w["fourier_feats.0.angular_speeds"]).abs().max()) + 2e-6)
    c.exact("cond.h1 = GELU(ff1 sin)", b.S("cond.h1"), F.cond_h1(w, sinb))
    pre = b.S("cond.pre")
    Tn = sig.shape[0]
    c.exact("cond.pre noise rows", pre[:Tn], F.cond_noise_pre(w, b.S("cond.h1")))
    c.exact("cond.pre label rows", pre[Tn:], F.cond_label_pre(w, label_rows.double()))
    y = b.S("cond.y")
    c.exact("cond.y", y, F.cond_y(w, pre))
    kv, wq, bwq = b.S("cond.kv"), b.S("cond.wq"), b.S("cond.bwq")
    for i in range(b.L):
        rkv, rwq, rbwq = F.cond_tables(w, y, i, b.H)
        c.exact(f"blk{i} cond.kv", kv[i], rkv)
        c.exact(f"blk{i} cond.wq", wq[i], rwq)
        c.exact(f"blk{i} cond.bwq", bwq[i], rbwq)
    b.kv, b.wq, b.bwq = kv, wq, bwq


def check_ends(b, x_src, out):
    c, w = b.c, b.w
    t0 = b.S("tokens0")
    c.round("tokens0 = embed(x)", t0, F.embed(w, x_src.double(), b.patch).reshape(-1, b.d))
    last = b.S(f"blk{b.L - 1}.mlp").view(b.B, b.N, b.d)
    ref = F.tail(w, last, b.C, b.patch).reshape(b.B, -1)
    c.exact("out = tail(tokens_final)", b.S("out"), ref)
    if out is not None:
        c.equal("caller's output = out stage", out.double().reshape(b.B, -1), b.S("out"))


def check_block(b, i):
    c, w, d, N, H, G, hid, B = b.c, b.w, b.d, b.N, b.H, b.G, b.hid, b.B
    p, s = f"{R.BLK}decoder_blocks.{i}.", f"blk{i}."
    S = lambda n: b.S(s + n)
    b0 = b.src if i == 0 else B
    M0, M = b0 * N, B * N
    x_in = S("x_in")
    c.equal(s + "x_in = previous stage", x_in, b.S("tokens0") if i == 0 else b.S(f"blk{i - 1}.mlp"))
    fold1, two_kernel = b.has(s + "ln1"), b.has(s + "qk")
    wqkv = S("wqkv")
    if fold1:
        slots = 2 if i == 0 else d // 96
        ps = S("ln1")[:, :slots]
        c.exact(s + "LN1 partial sums (of the stored rows)", ps, F.partial_sums(x_in, slots, i == 0))
        mean, rstd = F.stats_from_sums(ps, d)
        g1 = w[p + "norm1.weight"]
        want = F.bf16(g1 * w[p + "self_attention.qkv_linear.weight"])
        c.equal(s + "wqkv = bf16(gamma1 W)", wqkv, want)
        c.exact(s + "qkv_c1 = column sums of wqkv", S("qkv_c1"), wqkv.sum(-1))
        c.exact(s + "qkv_b1 = beta1 . W^T", S("qkv_b1"), w[p + "norm1.bias"] @ w[p + "self_attention.qkv_linear.weight"].T)
        qkv = F.folded_linear(x_in, wqkv, S("qkv_c1"), S("qkv_b1"), mean, rstd)
    else:
        xn1 = S("xn1")
        c.round(s + "xn1 = LN1(x)", xn1, R.ln_fwd(x_in, w[p + "norm1.weight"], w[p + "norm1.bias"])[0])
        c.equal(s + "wqkv = bf16(W)", wqkv, F.bf16(w[p + "self_attention.qkv_linear.weight"]))
        qkv = xn1 @ wqkv.T
    att = S("att")
    if two_kernel:
        qk, vt = S("qk"), S("vt")
        c.round(s + "QKV q | k", qk, qkv[:, :2 * d], K=d)
        v_eng = vt.permute(0, 2, 1).reshape(M0, d)                               # [samples, d, N] -> [M, d]
        c.round(s + "QKV V^T", v_eng, qkv[:, 2 * d:], K=d)
        q3, k3, v3 = qk[:, :d].view(b0, N, d), qk[:, d:].view(b0, N, d), v_eng.view(b0, N, d)
        exact, model = _attn_both(q3, k3, v3, H, False)
    else:   # fused: q | k | v are rounded to bf16 on their way into LDS (tld_gemm.hip, EPI_QKV_ATTN), then attention as in the two-kernel path
        q3, k3, v3 = F.split_qkv(qkv, b0, N)
        exact, model = _attn_both(q3, k3, v3, H, True)
    c.modelled(s + ("self-attention" if two_kernel else "fused QKV + self-attention"), att, exact.reshape(M0, d), F.bf16(model).reshape(M0, d), b0, heads=True)
    del exact, model, qkv
    # the row kernel: x1 = x + att (fanned out to both CFG halves in block 0 of a sampler step), cross-attention, statistics
    rep = B // b0
    xi3, at3 = x_in.view(b0, N, d).repeat(rep, 1, 1), att.view(b0, N, d).repeat(rep, 1, 1)
    x1, x2 = F.cross_row(xi3, at3, b.wq[i], b.bwq[i], b.kv[i][:, d:], b.nrow, b.lrow)
    c.exact(s + "sa = x + att", S("sa"), x1.reshape(M, d))
    ca = S("ca")
    c.round(s + "ca = sa + cross-attention", ca, x2.reshape(M, d), K=d)
    fold3 = b.has(s + "stats")
    wup = S("wup")
    if fold3:
        st = S("stats")
        ref = F.row_stats(ca)
        c.exact(s + "LN3 mean (of the stored row)", st[:, :1], ref[:, :1]); c.exact(s + "LN3 rstd", st[:, 1:], ref[:, 1:])
        g3, W = w[p + "norm3.weight"], w[p + "mlp.mlp.0.weight"].reshape(hid, d)
        c.equal(s + "wup = bf16(gamma3 W)", wup, F.bf16(g3 * W))
        c.exact(s + "up_c1 = column sums of wup", S("up_c1"), wup.sum(-1))
        c.exact(s + "up_b1 = bias + beta3 . W^T", S("up_b1"), w[p + "mlp.mlp.0.bias"] + w[p + "norm3.bias"] @ W.T)
        up = F.folded_linear(ca, wup, S("up_c1"), S("up_b1"), st[:, :1], st[:, 1:])
    else:
        xn3 = S("xn3")
        # (without the fold cross_row normalises the fp32 row it holds, before the store rounds it: tld_rows.hip, `if (fold3)` in phase C)
        c.round(s + "xn3 = LN3(sa + cross-attention)", xn3, R.ln_fwd(x2.reshape(M, d), w[p + "norm3.weight"], w[p + "norm3.bias"])[0])
        c.equal(s + "wup = bf16(W)", wup, F.bf16(w[p + "mlp.mlp.0.weight"].reshape(hid, d)))
        up = xn3 @ wup.T + w[p + "mlp.mlp.0.bias"]
    dww, dwb = w[p + "mlp.mlp.1.weight"].reshape(hid, 9), w[p + "mlp.mlp.1.bias"]
    hidt = S("hid")
    if b.has(s + "hid_pre"):
        pre = S("hid_pre")
        c.round(s + "up projection", pre, up, K=d)
        exact = F.dw_gelu(pre.view(B, N, hid), dww, dwb, G).reshape(M, hid)
        if G <= 16:      # whole-image kernel: fp32 taps, the 3e-7 erf (tld_common.h erf_as): exact, rounded once
            c.round(s + "depthwise + GELU (whole image)", hidt, exact)
        else:
            model = F.bf16(F.dw_gelu_model(pre.view(B, N, hid), dww, dwb, G, False)).reshape(M, hid)
            c.modelled(s + "depthwise + GELU (halved tables)", hidt, exact, model, B, pixels=True)
    else:   # fused: bf16(acc + bias) goes to LDS as an image, the conv runs on bf16 tap pairs, GELU by the polynomial
        exact = F.dw_gelu(up.view(B, N, hid), dww, dwb, G).reshape(M, hid)
        model = F.bf16(F.dw_gelu_model(F.bf16(up).view(B, N, hid), dww, dwb, G, True)).reshape(M, hid)
        c.modelled(s + "fused up projection + depthwise + GELU", hidt, exact, model, B, pixels=True)
        del model
    del exact, up
    wdown = S("wdown")
    c.equal(s + "wdown = bf16(W)", wdown, F.bf16(w[p + "mlp.mlp.3.weight"].reshape(d, hid)))
    mlp = S("mlp")
    if b.has(s + "splitk"):
        sl = S("splitk")
        ks = hid // sl.shape[0]
        for j in range(sl.shape[0]):
            c.exact(s + f"split-K slice {j}", sl[j], hidt[:, j * ks:(j + 1) * ks] @ wdown[:, j * ks:(j + 1) * ks].T)
        c.round(s + "mlp = ca + bias + slices (finisher)", mlp, ca + w[p + "mlp.mlp.3.bias"] + sl.sum(0))
    else:
        c.round(s + "mlp = ca + down projection", mlp, ca + hidt @ wdown.T + w[p + "mlp.mlp.3.bias"], K=hid)


def _attn_both(q3, k3, v3, H, fused):
    """(exact, model) of self-attention, a few samples at a time (the float64 probabilities of 4096 tokens are 1.6 GB per sample)."""
    B, N, _ = q3.shape
    step = max(1, (1 << 27) // (H * N * N))
    ex, mo = [], []
    for a in range(0, B, step):
        q, k, v = q3[a:a + step], k3[a:a + step], v3[a:a + step]
        ex.append(R.attn_fwd(q, k, v, H))
        mo.append(F.attn_model(F.bf16(q), F.bf16(k), F.bf16(v), H) if fused else F.attn_model(q, k, v, H))
    return torch.cat(ex), torch.cat(mo)


def _inputs(kw, B, seed):
    gen = torch.Generator().manual_seed(seed)
    S, C = kw["image_size"], kw["n_channels"]
    x = torch.randn(B, C, S, S, generator=gen)
    sigma = torch.rand(B, 1, generator=gen) * 0.9 + 0.05
    lab = torch.randn(B, 768, generator=gen) * 0.5
    zero = sorted({1 % B, B - 1})
    lab[zero] = 0
    return x, sigma, lab, zero


_PATHS = {}


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


def run_forward_case(name, io_dtype=torch.float32, blocks=None, case=None, checks=None, paths=None):
    """case: a row like those of CASES, run under the tag `name` (tests/test_gpu_forward_grids.py); checks: the Checks class; paths: where the launch-path
    masks go (this file's record otherwise)."""
    kw, batches, max_batch, env, lowlat = CASES[name] if case is None else case
    paths = _PATHS if paths is None else paths
    dev = _dev()
    m = _model(kw)
    if lowlat:
        m.set_low_latency(lowlat)
    _with_env(env, lambda: m.reserve(max_batch))          # the switches are read at tld_engine_create
    m.set_debug(True)
    try:
        for B in batches:
            x, sigma, lab, zero = _inputs(kw, B, 40 + B)
            xd, sd_, ld = (t.to(dev).to(io_dtype) for t in (x, sigma, lab))
            out = m(xd, sd_, ld)
            torch.cuda.synchronize()
            tag = name if len(batches) == 1 else f"{name}/{B}"
            if io_dtype != torch.float32:
                tag += "/" + str(io_dtype).split(".")[-1]
            b = Body(m, kw, tag, B, B, torch.arange(B), torch.arange(B) + B, zero, checks=checks)
            paths[tag] = b.paths
            check_cond(b, sd_.float().reshape(-1), ld.float())
            check_ends(b, xd.float(), out if io_dtype == torch.float32 else None)
            if io_dtype != torch.float32:      # the casts: inputs rounded by the caller, the output rounded once from the fp32 stage
                b.c.equal("output = cast(out stage)", out.double().reshape(B, -1), b.S("out").to(io_dtype).double())
            for i in (range(b.L) if blocks is None else blocks):
                check_block(b, i)
                torch.cuda.empty_cache()
            report(b.c)
    finally:
        m.set_debug(False)
        del m
        gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(CASES))
def test_forward_stages(name):
    run_forward_case(name)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_io_casts(dt):
    run_forward_case(IO_CASE, io_dtype=dt, blocks=(0,))


# ---- sampler steps ----------------------------------------------------------------------------------------------------------------------------
SAMPLERS = {   # name: (config, B, levels, debug steps)
    "tiny": (_cfg(128, 32, 3), 2, 6, (0, 1, 5)),
    "C1s": (_cfg(768, 32, 12), 64, 6, (0, 1, 5)),       # the 100M model, every block, layer-0 sharing on
}


def _check_trace_updates(c, what, x_start, tx0, txt, co, eps=None, z0=None, mask=None):
    """Every step's update from the traces alone: xt[i + 1] is a function of xt[i], x0[i], x0[i - 1] and the coefficients."""
    n = co.shape[0]
    xt = x_start.double()
    for i in range(n - 1):
        x0, xp = tx0[i].double(), (tx0[i - 1].double() if i else torch.zeros_like(xt))
        ref = F.update_from(xt, x0, xp, co[i], float(co[i + 1][0]), eps, z0, mask)
        c.exact(f"{what} update, step {i}", txt[i].double(), ref)
        xt = txt[i].double()


def _sampler(name, plus, from_image, masked=True, case=None, checks=None, paths=None):
    from transformer_latent_diffusion_amd import schedule
    kw, B, n_levels, steps = SAMPLERS[name] if case is None else case
    paths = _PATHS if paths is None else paths
    dev = _dev()
    m = _model(kw, seed=33)
    m.reserve(2 * B)
    m.set_debug(True)
    g = 3.0
    gen = torch.Generator().manual_seed(50 + B)
    S, C = kw["image_size"], kw["n_channels"]
    xT = torch.randn(B, C, S, S, generator=gen).to(dev)
    lab = (torch.randn(B, 768, generator=gen) * 0.5).to(dev)
    levels = schedule.noise_schedule(n_levels, 1)
    co = schedule.step_coefficients(levels, plus)
    n = co.shape[0]
    z0 = mask = None
    s0 = 1.0
    if from_image:
        z0 = (torch.randn(B, C, S, S, generator=gen) * 0.7).to(dev)
        s0 = 0.8
        if masked:     # a fractional mask with both exact ends
            mask = torch.rand(B, 1, S, S, generator=gen).to(dev)
            mask[:, :, : S // 4] = 1.0; mask[:, :, S // 2:] = 0.0
    tag = f"{name}/{'dpm' if plus else 'ddim'}{('/from+mask' if masked else '/from') if from_image else ''}"
    try:
        for step in steps:
            step = min(step, n - 1)
            m.set_debug_step(step)
            if from_image:
                lat, tx0, txt = m.sample_latents_from(xT, z0, lab, co, g, s0, mask=mask, sharp_f=0.1, bright_f=-0.05, trace=True)
            else:
                lat, tx0, txt = m.sample_latents(xT, lab, co, g, sharp_f=0.1, bright_f=-0.05, trace=True)
            torch.cuda.synchronize()
            nrow = torch.full((2 * B,), step)
            lrow = n + torch.cat([torch.arange(B), torch.full((B,), B)])
            b = Body(m, kw, f"{tag}/step{step}", 2 * B, B, nrow, lrow, zero_label=tuple(range(B, 2 * B)), checks=checks)
            paths[b.c.name] = b.paths
            c = b.c
            sig = torch.tensor([co[i][0] for i in range(n)], device=dev)
            check_cond(b, sig, torch.cat([lab, torch.zeros(1, 768, device=dev)]))
            x_t = b.S("step.x_t").view(B, C, S, S)
            start = F.start_mix(xT.double(), z0.double(), s0) if from_image else xT.double()
            if step == 0:
                c.exact("x_t entering step 0 = start (start_mix)", x_t, start)
            else:
                c.equal("x_t entering the step = trace", x_t, txt[step - 1].double())
                c.equal("x0_prev entering the step = trace", b.S("step.x0_prev").view(B, C, S, S), tx0[step - 1].double())
            check_ends(b, x_t, None)                     # block 0 up to att runs on the un-doubled batch: tokens0 has B samples
            for i in range(b.L):
                check_block(b, i)
            out2 = b.S("step.out")
            c.equal("step.out = out stage", out2, b.S("out"))
            x0 = F.cfg_combine(out2.view(2 * B, C, S, S), g)
            last = step == n - 1
            md, zd = (mask.double() if mask is not None else None), (z0.double() if from_image else None)
            if last:
                c.exact("final x0 = CFG (+ blend) + shifts", b.S("step.x0").view(B, C, S, S), F.final_x0(x0, 0.1, -0.05, zd, md))
                c.equal("returned latent = step.x0", lat.double().reshape(B, -1), b.S("step.x0"))
            else:
                c.exact("x0 = CFG combination", b.S("step.x0").view(B, C, S, S), x0)
                ref = F.update_from(x_t, b.S("step.x0").view(B, C, S, S), b.S("step.x0_prev").view(B, C, S, S), co[step], float(co[step + 1][0]),
                                    xT.double(), zd, md)
                c.exact("x_next = update" + (" (second order)" if plus and step > 0 else ""), b.S("step.x_next").view(B, C, S, S), ref)
            if step == steps[0]:
                _check_trace_updates(c, tag, start, tx0, txt, co.astype(np.float64), xT.double(), zd, md)
            report(c)
    finally:
        m.set_debug(False)
        del m
        gc.collect(); torch.cuda.empty_cache()


@pytest.mark.parametrize("name,plus", [("tiny", True), ("tiny", False), ("C1s", True), ("C1s", False)])
def test_sampler_steps(name, plus):
    _sampler(name, plus, False)


@pytest.mark.parametrize("name,plus,masked", [("tiny", True, True), ("tiny", True, False), ("tiny", False, True), ("tiny", False, False),
                                              ("C1s", True, True), ("C1s", False, False)])
def test_sampler_from_image_steps(name, plus, masked):
    _sampler(name, plus, True, masked)


# ---- the hook itself --------------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_launch_path():
    from transformer_latent_diffusion_amd import Denoiser
    for name in CASES:
        if not any(k == name or k.startswith(name + "/") for k in _PATHS):
            run_forward_case(name, blocks=())
    if not any(k.startswith("tiny/dpm/from+mask") for k in _PATHS):
        _sampler("tiny", True, True, True)
    if not any(k.startswith("tiny/ddim/from/") for k in _PATHS):
        _sampler("tiny", False, True, False)
    if not any(k.startswith("tiny/dpm/step") for k in _PATHS):
        _sampler("tiny", True, False)
    kw, B = FP8_PATH_CASE
    m = _model(kw)
    m.set_gemm_dtype("fp8")
    m.reserve(B)
    m.set_debug(True)
    x, sigma, lab, _ = _inputs(kw, B, 7)
    out = m(x.to(_dev()), sigma.to(_dev()), lab.to(_dev()))
    assert bool(torch.isfinite(out).all())
    _PATHS["fp8"] = m.debug_paths()
    m.set_debug(False)
    del m
    mask = 0
    for v in _PATHS.values():
        mask |= v
    names = Denoiser.PATH_NAMES
    for k, v in sorted(_PATHS.items()):
        _record(f"launch paths {k:28s} {v:#018x}")
    missing = [names[i] for i in range(len(names)) if names[i] is not None and not mask >> i & 1]
    print(f"launch paths reached: {bin(mask).count('1')} (mask {mask:#x}; CUs {torch.cuda.get_device_properties(_dev()).multi_processor_count})")
    assert not missing, "launch paths no case reaches: " + ", ".join(missing)


def test_read_stage_checks_numel_and_names():
    kw = _cfg(128, 32, 2)
    m = _model(kw)
    m.reserve(2)
    m.set_debug(True)
    x, sigma, lab, _ = _inputs(kw, 2, 9)
    m(x.to(_dev()), sigma.to(_dev()), lab.to(_dev()))
    assert m.stage_shape("blk1.ca") == (512, 128) and m.stage_shape("cond.kv") == (2, 4, 256)
    with pytest.raises(RuntimeError, match="status 3"):
        m.read_stage("blk1.ca", (511, 128))
    with pytest.raises(RuntimeError, match="status 2"):
        m.read_stage("blk2.ca", (512, 128))
    for old, new in (("blk0_sa", "blk0.sa"), ("blk0_ca", "blk0.ca"), ("blk0_mlp", "blk0.mlp"), ("tokens_final", "blk1.mlp"), ("cond_y", "cond.y")):
        assert np.array_equal(m.read_stage(old), m.read_stage(new))
    m.set_debug(False)
    with pytest.raises(RuntimeError, match="status 2"):
        m.read_stage("blk1.ca")


def test_debug_runs_are_reproducible_and_debug_off_computes_the_same():
    """Two debug forwards give bitwise equal stages and outputs; debug off gives bitwise the same output as debug on (forward and sampler)."""
    from transformer_latent_diffusion_amd import schedule
    kw = _cfg(768, 32, 2)
    dev = _dev()
    m = _model(kw)
    m.reserve(16)
    x, sigma, lab, _ = _inputs(kw, 8, 11)
    x, sigma, lab = x.to(dev), sigma.to(dev), lab.to(dev)
    co = schedule.step_coefficients(schedule.noise_schedule(6, 1), True)
    off = m(x, sigma, lab).clone()
    off_s = m.sample_latents(x, lab, co, 3.0).clone()
    m.set_debug(True)
    names = ["blk0.att", "blk0.ca", "blk0.hid", "blk1.ln1", "blk1.stats", "blk1.mlp", "cond.wq"]
    on1 = m(x, sigma, lab).clone()
    first = {n: m.read_stage(n) for n in names}
    on2 = m(x, sigma, lab).clone()
    for n in names:
        a, b2 = first[n], m.read_stage(n)
        assert np.array_equal(a.view(np.int32), b2.view(np.int32)), n
    on_s = m.sample_latents(x, lab, co, 3.0).clone()
    m.set_debug(False)
    off2 = m(x, sigma, lab).clone()
    assert torch.equal(off, on1) and torch.equal(on1, on2) and torch.equal(off, off2)
    assert torch.equal(off_s, on_s)


@pytest.mark.parametrize("fused", ["1", "0"])
def test_fp8_debug_off_computes_the_same(fused):
    """The same on an fp8 engine, quantising producers and separate passes: the operand snapshots, hid_pre and the poisoning of a8 / as8 change no output bit."""
    from transformer_latent_diffusion_amd import schedule
    kw = _cfg(768, 32, 2)
    dev = _dev()
    m = _model(kw)
    m.set_gemm_dtype("fp8")
    _with_env({"TLD_FP8_FUSED": fused}, lambda: m.reserve(16))
    x, sigma, lab, _ = _inputs(kw, 8, 11)
    x, sigma, lab = x.to(dev), sigma.to(dev), lab.to(dev)
    co = schedule.step_coefficients(schedule.noise_schedule(6, 1), True)
    off = m(x, sigma, lab).clone()
    off_s = m.sample_latents(x, lab, co, 3.0).clone()
    m.set_debug(True)
    names = ["blk0.a8_qkv.q", "blk0.a8_up.s", "blk1.a8_down.q", "blk1.a8_down.s", "blk1.hid_pre", "blk1.mlp"]
    on1 = m(x, sigma, lab).clone()
    first = {n: m.read_stage(n) for n in names}
    on2 = m(x, sigma, lab).clone()
    for n in names:
        assert np.isfinite(first[n]).all() and np.array_equal(first[n], m.read_stage(n)), n
    on_s = m.sample_latents(x, lab, co, 3.0).clone()
    m.set_debug(False)
    off2 = m(x, sigma, lab).clone()
    assert torch.equal(off, on1) and torch.equal(on1, on2) and torch.equal(off, off2)
    assert torch.equal(off_s, on_s)

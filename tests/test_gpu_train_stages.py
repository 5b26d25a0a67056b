"""GPU: the training step (csrc/tld_train.hip, tld_train_kernels.h, tld_train_attn.hip) stage by stage against float64, on the engine's own inputs.

tld_train_set_debug poisons the engine's buffers with NaN, keeps every stage of one forward_backward call and records the launch path of
every size-dependent dispatch.  Each transition below is recomputed in float64 (tests/train_stage_refs.py, held against autograd on the
host by tests/test_train_stage_refs_host.py) from the engine's snapshot of its inputs and the operands as the engine holds them -- the bf16
GEMM operand copies (blk<i>.wqkv ...), fp32 for everything else -- and compared with the engine's snapshot of its output.  Errors do not
pile up, so the bounds are per element, or per class where a kernel has intermediate roundings:

* EXACT (fp32 out, only the summation order or a few fp32 roundings differ: weight gradients from bf16 operands, column sums, LayerNorm
  dx / gamma / beta, position table, tall weight gradients, the small fp32 products, loss): |got - ref| <= TAIL_TOL max|ref| per element,
  TAIL_TOL = 2e-5 as in tests/test_gpu_vae_blocks.py.  The longest sums are 32768 rows: 64-row sequential chunks, then a fixed tree over
  512 partials.  A sum of n fp32 terms of size s in chunks of c has rounding error about 2^-24 s sqrt(n c / 2) (each add rounds at the
  size of its running sum), i.e. 2^-24 sqrt(c / 2) = 3.4e-7 of a result of size s sqrt(n); a column whose terms cancel below that size
  is held against max|ref| of the tensor, not its own value.  2e-5 leaves 50x for the worst element of a tensor.
* ROUND (the fp32 result of exact products rounded once to bf16: every GEMM with a bf16 output, the residual add, LayerNorm outputs, the
  unfused GELU' product and input gradient): |got - ref| <= 2^-8 |ref| + 2e-5 sqrt(max(K, 64) / 64) max|ref| per element -- half a bf16
  ulp is at most 2^-8 |ref|; the second term is the fp32 accumulation bound tests/test_gpu_gemm_epilogues.py derives.
* MEASURED (intermediate roundings or fast-math inside the kernel: both attentions, GELU / GELU' of the depthwise forward, the fused
  depthwise backward): relative rms over the whole tensor and over every class -- first / last row, the rows of the last partial
  256-row tile, each sample, corner / edge / interior / band-seam pixels, each (sample, head), dropped-label samples.  Bounds are at most
  twice the worst value measured on an MI355X over all cases (profiles/r10_train_stage_errors.txt), written beside each constant.

* MODELLED (the attention backward, beside its MEASURED bound): dq, dk and dv per class of tests/test_gpu_attn_bwd_classes.py -- each (sample, head),
  full / partial blocks, the half-outside tile, each owning wave -- against twice the error of the float64 rounding model
  (train_stage_refs.attn_bwd_model, fp32-gradient form: the step passes its fp32 residual gradient) over the same member.  On an MI355X measured equals
  the yardstick to three digits at every case (profiles/r11_attn_bwd_classes.txt, section 3).

Every compared tensor is first checked for NaN / Inf (the poison), with the count in the message.
Every case holds its whole mask of tld_train_debug_paths against the plan's prediction (train_plan_ref.expected_mask: test_forward_stages and the TN-off
test).  CASES reach every launch path: test_cases_reach_every_launch_path holds the union of the masks against the full mask, and -- the one
"masked" bit standing for several kernel pairs -- the (mode, waves, masked) instantiation of the attention backward of every product grid.
Cases G4 ... G60 (d = 128, one block) run every grid the other cases leave out; they came after the mutation table below.

The checks bite.  Eight numeric, in-bounds mutations of the kernels, one build each, each run once on an MI355X: this file, then the end-to-end
gradient tests of tests/test_gpu_train.py (test_forward_backward_vs_reference_step g15 / g17, test_64_token_step..., test_wide_model_gradients...: "old 4").
Failing tests of this file (of 31; F = test_forward_stages, B = test_backward_stages, T = the TN-off test), the worst comparison against its bound,
and the old file's result:
  1 ln_bwd_q4_kernel, the mean-of-(dy gamma xhat) term with the neighbouring row's rstd on the last row of each 32-row workgroup:
      5 fail -- B[A, A', C, D, G] (the q4 widths 256 / 512 / 768); LayerNorm dx, EXACT: 9.6e-3 ... 5.2e-2 against 2e-5.  Old 4: all pass
  2 cross_bwd_kernel, p0 and 1 - p0 swapped for the last head: 9 fail -- B[every case]; dkv per conditioning token 0.21 ... 0.86 against 2.5e-7.  Old 4: all fail.
      dqc = p0 (1 - p0) (...) is symmetric under the swap and does not move: the mutation is visible in dkv only
  3 dwconv_bwd_img_kernel, one input-gradient tap dropped on the last image column: 4 fail -- B[A, A', D], T[A] (the fused form's cases); dh of
      the last row 0.47 ... 0.56 against 4.9e-3, whole tensor 8e-2 against 4.6e-3, the fused up bias 2.4e-2 against 7.9e-4.  As worded in
      the issue, the (+1, +1) tap, the mutation changes nothing: on the last column that neighbour lies outside the image and is zero; the
      tap dropped here is the one that reads dhc[y - 1][x - 1].  Old 4: 2 fail (g15, wide model), 2 pass
  4 colsum4_partial, the last 64-row chunk of a launch skipped: 7 fail -- B[A, A', C, D, G], T[A, C] (rows >= 4096); bias gradients 6.5e-3 ...
      6.1e-2 against 2e-5.  Old 4: all pass (no old test has 4096 rows at these widths)
  5 resid_add_ln_q4_kernel<3>, variance divided by d - 1: 2 fail -- F[A, A'] (d = 768); rstd 6.5e-4 against 2e-5, LayerNorm output 1.15 of its
      per-element rounding bound.  Old 4: all pass
  6 pos_grad_kernel, sample 0 left out: 9 fail -- B[every case]; position table 6.1e-2 (batch 128) ... 0.83 against 2e-5.  Old 4: all fail (batches of 2 ... 4)
  7 the x phi(x) term of GELU' dropped where |x| < 1/8: 9 fail -- F[every case]; hc 2.9e-2 whole / 3.6e-2 ... 3.8e-2 worst class against 3.3e-3 /
      3.4e-3.  GELU' is computed once, by gelu_pair in the forward dwconv_kernel, and stored as hc; gelu_bwd_kernel and the fused backward
      only multiply by it, so that is where the term was dropped.  Old 4: all pass
  8 the per-block k | v stride taken from batch instead of max_batch: 3 fail -- F[A'], B[A'] and the gradient test of A' (blk1.kvc keeps the NaN poison,
      111 comparisons not finite); no other case, as required.  Old 4: 2 fail (g17 and the wide model, which run fewer samples than their engine's max_batch), 2 pass
Every MEASURED bound is below the effect of each mutation on its transition by 6x or more (the smallest margin: mutation 7, hc whole tensor).
Mutations 1, 4, 5 and 7 pass the old file and fail here; the issue's estimate that 6 would also pass the old file did not hold at its small batches.
Wall time on an MI355X: this file 28 s run alone (31 tests; case A takes most of it), 22 s inside the whole suite; tests/test_gpu_train.py, unchanged
from the parent, 12 s inside the whole suite (27 tests)."""
import gc
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_plan_ref
import train_stage_refs as R
from test_gpu_attn_bwd_classes import GRIDS, compare as attn_bwd_compare, dispatch as attn_bwd_dispatch
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TAIL_TOL = 2e-5           # EXACT: max |got - ref| / max|ref|
ROUND_C = 2e-5            # ROUND: |got - ref| <= 2^-8 |ref| + ROUND_C sqrt(max(K, 64) / 64) max|ref|
# MEASURED: worst relative rms over the classes, bound <= 2 x the worst value measured on an MI355X (in the comment)
MEASURED = {                         # (whole tensor, worst class)
    "attn": (3.7e-3, 3.9e-3),                 # self-attention forward: measured 1.88e-3 (case C) / 1.96e-3 (case C, last row)
    "cross.cr": (3.3e-3, 3.8e-3),             # cross-attention output: measured 1.66e-3 (case B) / 1.92e-3 (case A', a (sample, head))
    "cross.p0": (1.4e-7, 8.4e-6),             # its saved p0 and 1 - p0 (fp32, fast exp): measured 7.36e-8 (case I) / 4.23e-6 (case I, one row of 1 - p0 near 0)
    "dw.hc": (3.3e-3, 3.4e-3),                # GELU'(depthwise) as stored: measured 1.66e-3 (case B) / 1.71e-3 (case B, first row)
    "dw.gl": (3.3e-3, 3.6e-3),                # GELU(depthwise): measured 1.67e-3 (case B) / 1.85e-3 (case I, last row)
    "attn_bwd": (1.5e-2, 2.3e-2),             # dq | dk | dv: measured 7.61e-3 (case B, dq) / 1.20e-2 (case A, dq of one (sample, head))
    "cross_bwd.dqc": (3.3e-3, 3.8e-3),        # measured 1.68e-3 (case I) / 1.91e-3 (case F, first row)
    "cross_bwd.dkv": (2.3e-7, 2.5e-7),        # fp32 sums over the tokens, per conditioning token: measured 1.20e-7 / 1.26e-7 (case I)
    "dw_bwd_fused.dh": (4.6e-3, 4.9e-3),      # dh from (dg, hc, h), dhc rounded to bf16 inside the kernel: measured 2.33e-3 / 2.45e-3 (case A', first row)
    "dw_bwd_fused.params": (7.9e-4, 1.9e-3),  # its depthwise weight / bias and up bias sums: measured 3.95e-4 (case A') / 9.66e-4 (case A, the last channel's nine taps)
}

# name: (config, batch, max_batch)
def _cfg(d, image, blocks, patch=2, C=4, mult=4):
    return dict(image_size=image, noise_embed_dims=256, patch_size=patch, embed_dim=d, dropout=0, n_layers=blocks, text_emb_size=768, n_channels=C,
                mlp_multiplier=mult)


CASES = {
    "A": (_cfg(768, 32, 2), 128, 128),            # the trained size: M = 32768, 384-wide tile, split weight gradients, colsum4, fused depthwise backward
    "A'": (_cfg(768, 32, 2), 37, 128),            # batch < max_batch strides, M = 9472
    "B": (_cfg(192, 24, 2), 3, 3),                # M = 432 (not a multiple of 64), generic LN kernels, unfused depthwise backward at G <= 16
    "C": (_cfg(256, 64, 1), 5, 5),                # two-kernel attention backward, banded depthwise, q4<1>
    "D": (_cfg(512, 64, 1, patch=4), 20, 20),     # plain embedding kernel, tail_dx4<64>, q4<2>
    "E": (_cfg(1024, 16, 1, C=3, mult=2), 8, 8),  # generic tail / tall_dw_partial, resid q4<4> with the generic LN backward, embedding LDS<4>
    "F": (_cfg(320, 40, 1, C=8), 2, 2),           # tail_dx4<32>, masked attention kernels, M = 800
    "G": (_cfg(256, 128, 1), 2, 2),               # four depthwise bands, 16 key blocks
    "I": (_cfg(192, 16, 1), 2, 2),                # M = 128 with a width the untransposed weight gradient refuses: the transposing form, one run
}
# every other product grid G x G at the narrowest width (d = 128, one block): with B (144), C (1024), A (256), F (400), G (4096) and E (64) the
# attention backward runs the instantiation of every grid the trainer accepts (test_cases_reach_every_launch_path), and the depthwise bands,
# the position table and the tail run at those grids too
for _G in (4, 24, 28, 36, 40, 44, 48, 52, 56, 60):
    CASES[f"G{_G}"] = (_cfg(128, 2 * _G, 1), 1 if _G >= 52 else 2, 1 if _G >= 52 else 2)
TN_OFF_CASES = ("A", "C")                         # case H: the transposing weight gradient with split runs (TLD_TRAIN_TN_WGRAD=0, fresh process)


def _atoi(text):
    """C's atoi, as tld_train_create reads TLD_TRAIN_TN_WGRAD: leading blanks, a sign, digits; anything else ends the number (none: 0)."""
    import re
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


class _Tracked(dict):
    def __init__(self, *a):
        super().__init__(*a)
        self.read = set()

    def __getitem__(self, k):
        self.read.add(k)
        return super().__getitem__(k)


# ---- running a case -------------------------------------------------------------------------------------------------------------------
class Run:
    def __init__(self, name):
        from transformer_latent_diffusion_amd import DenoiserConfig, Trainer
        from transformer_latent_diffusion_amd.weights import synth_state_dict
        kw, self.B, max_batch = CASES[name]
        self.name, self.cfg = name, DenoiserConfig(**kw)
        self.dev = _dev()
        sd = synth_state_dict(self.cfg, 31)
        self.tr = Trainer(self.cfg, device=self.dev, state_dict={k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, max_batch=max_batch,
                          keep_ema=False, use_graph=False)
        c = kw
        self.d, self.L, self.patch, self.C = c["embed_dim"], c["n_layers"], c["patch_size"], c["n_channels"]
        self.H, self.G = self.d // 64, c["image_size"] // c["patch_size"]
        self.N, self.hid = self.G * self.G, self.d * c["mlp_multiplier"]
        self.M = self.B * self.N
        gen = torch.Generator().manual_seed(32 + self.B)
        S, B = c["image_size"], self.B
        x = torch.randn(B, self.C, S, S, generator=gen) * 0.8
        noise = torch.randn(B, self.C, S, S, generator=gen)
        nl = torch.rand(B, generator=gen, dtype=torch.float64) * 0.9 + 0.05
        lab = torch.randn(B, 768, generator=gen) * 0.5
        self.dropped = sorted({1 % B, B - 1})
        lab[self.dropped] = 0
        from transformer_latent_diffusion_amd.train import mix_noise
        self.inputs = (mix_noise(x, nl, noise).to(self.dev), nl.float().to(self.dev), lab.to(self.dev), x.to(self.dev))
        self.tr.set_debug(True)
        self.loss, self.pred = self.tr.forward_backward(*self.inputs)
        torch.cuda.synchronize()
        self.paths = self.tr.debug_paths()
        # the plan's prediction of that mask (csrc/tld_train_plan.h through its restatement), for this device and this process's TLD_TRAIN_TN_WGRAD
        self.expected_paths = train_plan_ref.expected_mask(kw, self.B, max_batch, torch.cuda.get_device_properties(self.dev).multi_processor_count,
                                                           _atoi(os.environ.get("TLD_TRAIN_TN_WGRAD", "1")) != 0)
        self.w = {k: v.double() for k, v in self.tr.state_dict().items()}
        self.grads = _Tracked({k: v.double() for k, v in self.tr.grad_dict().items()})      # remembers which tensors a check has read
        self.backward_done = False
        self.rows = []                                 # (transition, kind, value, bound)
        self.fail = []

    def S(self, name):
        return self.tr.read_stage(name).to(self.dev).double()

    # ---- comparisons ----
    def _finite(self, what, got):
        bad = int((~torch.isfinite(got)).sum())
        if bad:
            self.fail.append(f"{self.name} {what}: {bad} of {got.numel()} values are NaN / Inf")
            self.rows.append((what, "finite", float("inf"), 0.0))
        return bad == 0

    def _note(self, what, kind, val, bound):
        self.rows.append((what, kind, val, bound))
        if bound is not None and not val <= bound:
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

    def classes(self, got, ref, heads=False, pixels=True):
        """Worst relative rms over the whole tensor and every row / sample / pixel / head class of a [M, F] (or [B-rows, F]) tensor."""
        B, N, G, H = self.B, self.N, self.G, self.H
        e2, r2 = (got - ref) ** 2, ref ** 2
        F_ = e2.shape[-1]
        whole = float(r2.sum())
        out = {}

        def add(tag, es, rs):
            es, rs = es.reshape(-1), rs.reshape(-1)
            ok = rs > 1e-6 * whole / max(rs.numel(), 1)          # a class whose reference is (numerically) zero is held to the whole tensor's size
            rel = torch.where(ok, es / rs.clamp_min(1e-300), es / (whole / max(rs.numel(), 1)))
            out[tag] = math.sqrt(float(rel.max()))
        add("whole", e2.sum(), r2.sum())
        rows = e2.shape[0]
        add("first row", e2[0].sum(), r2[0].sum()); add("last row", e2[-1].sum(), r2[-1].sum())
        if rows % 256:
            t = rows - rows % 256
            add("last partial tile", e2[t:].sum(), r2[t:].sum())
        if rows == B * N:
            e3, r3 = e2.view(B, N, F_), r2.view(B, N, F_)
            add("sample", e3.sum((1, 2)), r3.sum((1, 2)))
            add("dropped-label samples", e3[self.dropped].sum(), r3[self.dropped].sum())
            if pixels:
                yy, xx = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
                ey, ex = (yy == 0) | (yy == G - 1), (xx == 0) | (xx == G - 1)
                masks = {"corner": ey & ex, "edge": ey ^ ex, "interior": ~(ey | ex), "last column": xx == G - 1}
                if G > 16:          # the depthwise kernels work in bands of dwconv_band_rows(G) = min(G, 16) image rows (tld_train_kernels.h)
                    masks["band seam"] = (yy % 16 == 15) | (yy % 16 == 0)
                for tag, m in masks.items():
                    m = m.reshape(-1).to(e2.device)
                    add(tag, e3[:, m].sum(), r3[:, m].sum())
            if heads and F_ % (64 * H) == 0:
                k = F_ // (64 * H)
                add("(sample, head)", e3.view(B, N, k, H, 64).sum((1, 2, 4)), r3.view(B, N, k, H, 64).sum((1, 2, 4)))
        return out

    def meas(self, what, key, got, ref, **kw):
        assert got.shape == ref.shape, (what, got.shape, ref.shape)
        if self._finite(what, got):
            cl = self.classes(got, ref, **kw)
            whole_bound, class_bound = MEASURED[key]
            self._note(f"{what} (whole)", "meas:" + key + ":whole", cl.pop("whole"), whole_bound)
            tag = max(cl, key=cl.get)
            self._note(f"{what} ({tag})", "meas:" + key + ":class", cl[tag], class_bound)


_RUN = {}
_PATHS = {}


def run_case(name):
    """One engine and its snapshots alive at a time (case A holds a few GB)."""
    if name not in _RUN:
        for k in list(_RUN):
            _RUN.pop(k).tr.set_debug(False)
        gc.collect(); torch.cuda.empty_cache()
        _RUN[name] = Run(name)
        _PATHS[name] = _RUN[name].paths
    return _RUN[name]


def report(r, start):
    for what, kind, val, bound in r.rows[start:]:
        print(f"case {r.name:2s} {what:48s} {kind:22s} {val:.3e}  bound {bound if bound is None else format(bound, '.1e')}")
    assert not r.fail, "\n".join(r.fail)


# ---- the transitions -------------------------------------------------------------------------------------------------------------------
def forward_ends(r):
    w, d, B, N, M = r.w, r.d, r.B, r.N, r.M
    xn, nl, lab, x = (t.double() for t in r.inputs)
    ang = w["fourier_feats.0.angular_speeds"].to(r.dev).double()
    sinb = r.S("sinb")
    ref = R.sinusoid(nl, ang)
    if r._finite("cond.sinusoid", sinb):   # the fp32 product sigma * speed is rounded before sinf: 2^-24 |a| on the argument, + sinf's own 1e-6
        r._note("cond.sinusoid", "derived", float((sinb - ref).abs().max()), 2.0 ** -23 * float((nl.view(-1, 1) * ang).abs().max()) + 2e-6)
    h1 = R.linear_fwd(sinb, w["fourier_feats.1.weight"], w["fourier_feats.1.bias"])
    r.exact("cond.h1", r.S("h1"), h1)
    r.exact("cond.gelu", r.S("g1v"), R.gelu(r.S("h1")))
    ycat = torch.stack([R.linear_fwd(r.S("g1v"), w["fourier_feats.3.weight"], w["fourier_feats.3.bias"]),
                        R.linear_fwd(lab, w["label_proj.weight"], w["label_proj.bias"])], dim=1).reshape(2 * B, d)
    r.exact("cond.ycat", r.S("ycat"), ycat)
    y, ym, yr = R.ln_fwd(r.S("ycat"), w["norm.weight"], w["norm.bias"])
    r.exact("cond.y", r.S("y"), y)
    r.exact("cond.y stats", r.S("yst"), torch.cat([ym, yr], dim=1))
    ye = r.S("y")
    for tok in (0, 1):
        r.exact(f"cond.y token {tok}", ye[tok::2], y[tok::2])
    for i in range(r.L):                  # all blocks' k | v in the one batched launch (per-block stride: max_batch)
        r.exact(f"blk{i}.kvc", r.S(f"blk{i}.kvc"), R.linear_fwd(ye, w[f"{R.BLK}decoder_blocks.{i}.cross_attention.kv_linear.weight"]))
    pe = R.BLK + "patchify_and_embed."
    pd = r.C * r.patch ** 2
    p16 = R.linear_fwd(R.patchify(xn, r.patch), w[pe + "0.weight"].reshape(pd, -1), w[pe + "0.bias"]).reshape(M, pd)
    r.exact("embed.p16", r.S("p16"), p16)
    p16n, m1, r1 = R.ln_fwd(r.S("p16"), w[pe + "2.weight"], w[pe + "2.bias"])
    r.exact("embed.p16n", r.S("p16n"), p16n)
    r.exact("embed.est1 mean", r.S("est1")[:, :1], m1); r.exact("embed.est1 rstd", r.S("est1")[:, 1:], r1)
    r.exact("embed.e", r.S("e"), R.linear_fwd(r.S("p16n"), w[pe + "3.weight"], w[pe + "3.bias"]))
    en, m2, r2 = R.ln_fwd(r.S("e"), w[pe + "4.weight"], w[pe + "4.bias"])
    r.exact("embed.est2 mean", r.S("est2")[:, :1], m2); r.exact("embed.est2 rstd", r.S("est2")[:, 1:], r2)
    x0 = (en.view(B, N, d) + w[R.BLK + "pos_embed.weight"][:N]).reshape(M, d)
    r.round("embed.x0", r.S("blk0.x1"), x0)
    # tail
    out = R.linear_fwd(r.S("xfin"), w[R.BLK + "out_proj.0.weight"], w[R.BLK + "out_proj.0.bias"]).view(B, N, pd)
    r.exact("tail.pred", r.pred.double(), R.unpatchify(out, r.C, r.patch))
    loss, dout, row = R.mse_fwd(out, R.patchify(x, r.patch))
    r.exact("tail.dout", r.S("dout"), dout.reshape(M, pd))
    r.exact("tail.row_loss", r.S("row_loss"), row.reshape(M))
    r.exact("tail.loss", r.loss.double().view(1), loss.view(1))


def forward_block(r, i):
    w, d, B, N, M, H, G, hid = r.w, r.d, r.B, r.N, r.M, r.H, r.G, r.hid
    p, s = f"{R.BLK}decoder_blocks.{i}.", f"blk{i}."
    S = lambda n: r.S(s + n)
    for op, src in (("wqkv", "self_attention.qkv_linear.weight"), ("wq", "cross_attention.q_linear.weight"), ("wup", "mlp.mlp.0.weight"),
                    ("wdown", "mlp.mlp.3.weight")):       # the operand copies are the bf16 rounding of the parameters, and their transposes
        ww = S(op)
        want = w[p + src].reshape(ww.shape).float().bfloat16().double()
        if not torch.equal(ww, want) or not torch.equal(S(op + "_t"), want.T):
            r.fail.append(f"{r.name} {s}{op}: the bf16 operand copy or its transpose differs from bf16(parameter)")

    def ln(xname, aname, stname, k):
        a, m, rs = R.ln_fwd(S(xname), w[p + f"norm{k}.weight"], w[p + f"norm{k}.bias"])
        st = S(stname)
        r.exact(s + f"ln{k} mean", st[:, :1], m); r.exact(s + f"ln{k} rstd", st[:, 1:], rs)
        r.round(s + f"ln{k} out", S(aname), a)
    x1 = S("x1")
    if i > 0:
        r.round(s + "x1 = x3 + o (previous block)", x1, r.S(f"blk{i - 1}.x3") + r.S(f"blk{i - 1}.o"))
    ln("x1", "a1", "st1", 1)
    qkv = R.linear_fwd(S("a1"), S("wqkv"))
    qk, vt = S("qk"), S("vt")
    r.round(s + "qkv q | k", qk, qkv[:, :2 * d], K=d)
    v_eng = vt.permute(0, 3, 1, 2).reshape(M, d)                                   # [B, H, 64, N] -> [M, d]
    r.round(s + "qkv V^T", v_eng, qkv[:, 2 * d:], K=d)
    q3, k3, v3 = qk[:, :d].view(B, N, d), qk[:, d:].view(B, N, d), v_eng.view(B, N, d)
    r.meas(s + "self-attention", "attn", S("att"), R.attn_fwd(q3, k3, v3, H).reshape(M, d), heads=True)
    r.round(s + "x2 = x1 + att", S("x2"), x1 + S("att"))
    ln("x2", "a2", "st2", 2)
    r.round(s + "q projection", S("qc"), R.linear_fwd(S("a2"), S("wq")), K=d)
    cr, p0 = R.cross_fwd(S("qc").view(B, N, d), S("kvc").view(B, 2, 2 * d), H)
    r.meas(s + "cross-attention cr", "cross.cr", S("cr"), cr.reshape(M, d), heads=True)
    r.meas(s + "cross-attention p0", "cross.p0", S("p0"), p0.reshape(M, H))
    r.meas(s + "cross-attention 1 - p0", "cross.p0", 1 - S("p0"), 1 - p0.reshape(M, H))
    r.round(s + "x3 = x2 + cr", S("x3"), S("x2") + S("cr"))
    ln("x3", "a3", "st3", 3)
    r.round(s + "up projection", S("h"), R.linear_fwd(S("a3"), S("wup"), w[p + "mlp.mlp.0.bias"]), K=d)
    pre = R.dwconv_fwd(S("h").view(B, N, hid), w[p + "mlp.mlp.1.weight"].reshape(hid, 9), w[p + "mlp.mlp.1.bias"], G).reshape(M, hid)
    r.meas(s + "depthwise + GELU (gl)", "dw.gl", S("gl"), R.gelu(pre))
    r.meas(s + "depthwise + GELU' (hc)", "dw.hc", S("hc"), R.gelu_grad(pre))
    del pre
    r.round(s + "down projection", S("o"), R.linear_fwd(S("gl"), S("wdown"), w[p + "mlp.mlp.3.bias"]), K=hid)
    if i == r.L - 1:
        r.round("xfin = x3 + o", r.S("xfin"), S("x3") + S("o"))


def _gin(r, i):
    return "gxb.tail" if i == r.L - 1 else f"blk{i + 1}.gxb.ln1"


def backward_block(r, i, weights_only=False):
    w, g, d, B, N, M, H, G, hid = r.w, r.grads, r.d, r.B, r.N, r.M, r.H, r.G, r.hid
    p, s = f"{R.BLK}decoder_blocks.{i}.", f"blk{i}."
    S = lambda n: r.S(s + n)
    fused = bool(r.paths >> 22 & 1)
    go = r.S(_gin(r, i))
    r.exact(s + "down bias", g[p + "mlp.mlp.3.bias"], go.sum(0))
    r.exact(s + "down weight", g[p + "mlp.mlp.3.weight"].reshape(d, hid), go.T @ S("gl"))
    dg, hc, h, dh = S("dg"), S("hc"), S("h"), S("dh")
    dww = w[p + "mlp.mlp.1.weight"].reshape(hid, 9)
    if not weights_only:
        r.exact(s + "gx at block entry = bf16 copy", go, r.S("gx.tail" if i == r.L - 1 else f"blk{i + 1}.gx.ln1").float().bfloat16().double())
        r.exact(s + "gx.in", S("gx.in"), r.S("gx.tail" if i == r.L - 1 else f"blk{i + 1}.gx.ln1"))
        r.round(s + "dg = go Wdown", dg, go @ S("wdown"), K=d)
    if fused:           # one kernel from (dg, hc, h) to dh and the three parameter gradients; dhc = bf16(dg hc) stays in LDS
        dh_ref, dw_ref, db_ref = R.dwconv_bwd((dg * hc).view(B, N, hid), h.view(B, N, hid), dww, G)
        if not weights_only:
            r.meas(s + "fused depthwise backward dh", "dw_bwd_fused.dh", dh, dh_ref.reshape(M, hid))
        r.meas(s + "fused depthwise weight", "dw_bwd_fused.params", g[p + "mlp.mlp.1.weight"].reshape(hid, 9), dw_ref, pixels=False)
        r.meas(s + "fused depthwise bias", "dw_bwd_fused.params", g[p + "mlp.mlp.1.bias"].view(1, hid), db_ref.view(1, hid), pixels=False)
        r.meas(s + "fused up bias", "dw_bwd_fused.params", g[p + "mlp.mlp.0.bias"].view(1, hid), dh_ref.reshape(M, hid).sum(0).view(1, hid), pixels=False)
    else:
        dhc = S("dhc")
        dh_ref, dw_ref, db_ref = R.dwconv_bwd(dhc.view(B, N, hid), h.view(B, N, hid), dww, G)
        if not weights_only:
            r.round(s + "dhc = dg GELU'", dhc, dg * hc)
            r.round(s + "depthwise input gradient dh", dh, dh_ref.reshape(M, hid))
        r.exact(s + "depthwise weight", g[p + "mlp.mlp.1.weight"].reshape(hid, 9), dw_ref)
        r.exact(s + "depthwise bias", g[p + "mlp.mlp.1.bias"], db_ref)
        r.exact(s + "up bias", g[p + "mlp.mlp.0.bias"], dh.sum(0))
    del dh_ref, dg, hc, h
    r.exact(s + "up weight", g[p + "mlp.mlp.0.weight"].reshape(hid, d), dh.T @ S("a3"))
    r.exact(s + "q weight", g[p + "cross_attention.q_linear.weight"], S("dqc").T @ S("a2"))
    r.exact(s + "kv weight", g[p + "cross_attention.kv_linear.weight"], S("dkv").T @ r.S("y"))
    r.exact(s + "qkv weight", g[p + "self_attention.qkv_linear.weight"], S("dqkv").T @ S("a1"))
    for k, dyn, gin in ((3, "da3", "gx.in"), (2, "da2", "gx.ln3"), (1, "da1", "gx.ln2")):
        st = S(f"st{k}")
        dx, dgam, dbet = R.ln_bwd(S(dyn), S(f"x{k}"), st[:, :1], st[:, 1:], w[p + f"norm{k}.weight"])
        r.exact(s + f"norm{k} weight", g[p + f"norm{k}.weight"], dgam)
        r.exact(s + f"norm{k} bias", g[p + f"norm{k}.bias"], dbet)
        if not weights_only:
            r.exact(s + f"LN{k} backward gx", S(f"gx.ln{k}"), S(gin) + dx)
    if weights_only:
        return
    r.round(s + "da3 = dh Wup", S("da3"), dh @ S("wup"), K=hid)
    del dh
    dqc, dkv = R.cross_bwd(S("gx.ln3").view(B, N, d), S("qc").view(B, N, d), S("kvc").view(B, 2, 2 * d), H)
    r.meas(s + "cross-attention backward dqc", "cross_bwd.dqc", S("dqc"), dqc.reshape(M, d), heads=True)
    dkv_e, dkv = S("dkv"), dkv.reshape(2 * B, 2 * d)
    for tok in (0, 1):
        r.meas(s + f"cross-attention backward dkv token {tok}", "cross_bwd.dkv", dkv_e[tok::2], dkv[tok::2], pixels=False)
    r.round(s + "da2 = dqc Wq", S("da2"), S("dqc") @ S("wq"), K=d)
    qk = S("qk")
    v3 = S("vt").permute(0, 3, 1, 2).reshape(B, N, d)
    dqkv = torch.cat(R.attn_bwd(qk[:, :d].view(B, N, d), qk[:, d:].view(B, N, d), v3, S("gx.ln2").view(B, N, d), H), dim=-1).reshape(M, 3 * d)
    r.meas(s + "attention backward dqkv", "attn_bwd", S("dqkv"), dqkv, heads=True)
    for j, nm in enumerate(("dq", "dk", "dv")):
        r.meas(s + "attention backward " + nm, "attn_bwd", S("dqkv")[:, j * d:(j + 1) * d], dqkv[:, j * d:(j + 1) * d], heads=True)
    # MODELLED: per class of tests/test_gpu_attn_bwd_classes.py against the rounding model, in the form of the instantiation the step runs
    # (TG = float: the engine passes its fp32 residual gradient, so delta = dO . O takes dO unrounded)
    model = torch.stack(R.attn_bwd_model(qk[:, :d].view(B, N, d), qk[:, d:].view(B, N, d), v3, S("att").view(B, N, d), S("gx.ln2").view(B, N, d), H, False))
    r.fail += attn_bwd_compare(f"case {r.name} {s}attention backward", S("dqkv").view(B, N, 3 * d), dqkv.view(B, N, 3, d).permute(2, 0, 1, 3).contiguous(), model, H,
                               attn_bwd_dispatch(N)[1], N)
    del model
    r.round(s + "da1 = dqkv Wqkv", S("da1"), S("dqkv") @ S("wqkv"), K=3 * d)
    if i > 0:
        r.round(s + "gxb = bf16(gx)", S("gxb.ln1"), S("gx.ln1"))


def backward_ends(r):
    w, g, d, B, N, M = r.w, r.grads, r.d, r.B, r.N, r.M
    xn, nl, lab, x = (t.double() for t in r.inputs)
    pd = r.C * r.patch ** 2
    Wout = w[R.BLK + "out_proj.0.weight"]
    dout = r.S("dout")
    r.exact("tail dx (gx)", r.S("gx.tail"), dout @ Wout)
    r.round("tail dx (gxb)", r.S("gxb.tail"), dout @ Wout)
    r.exact("out_proj weight", g[R.BLK + "out_proj.0.weight"], dout.T @ r.S("xfin"))
    r.exact("out_proj bias", g[R.BLK + "out_proj.0.bias"], dout.sum(0))
    dy = sum(r.S(f"blk{i}.dkv") @ w[f"{R.BLK}decoder_blocks.{i}.cross_attention.kv_linear.weight"] for i in range(r.L))
    r.exact("dL/dy over the blocks", r.S("dy"), dy)
    gx = r.S("blk0.gx.ln1")
    pos = torch.zeros_like(w[R.BLK + "pos_embed.weight"])
    pos[:N] = gx.view(B, N, d).sum(0)
    r.exact("position table", g[R.BLK + "pos_embed.weight"], pos)
    pe = R.BLK + "patchify_and_embed."
    st2, st1 = r.S("est2"), r.S("est1")
    de, dgam, dbet = R.ln_bwd(gx, r.S("e"), st2[:, :1], st2[:, 1:], w[pe + "4.weight"])
    r.exact("embed LN2 backward de", r.S("de"), de)
    r.exact("embed LN2 weight", g[pe + "4.weight"], dgam); r.exact("embed LN2 bias", g[pe + "4.bias"], dbet)
    de = r.S("de")
    r.exact("embed linear bias", g[pe + "3.bias"], de.sum(0))
    r.exact("embed linear dx (dpn)", r.S("dpn"), de @ w[pe + "3.weight"])
    r.exact("embed linear weight", g[pe + "3.weight"], de.T @ r.S("p16n"))
    dp16, dgam, dbet = R.ln_bwd(r.S("dpn"), r.S("p16"), st1[:, :1], st1[:, 1:], w[pe + "2.weight"])
    r.exact("embed LN1 backward dp16", r.S("dp16"), dp16)
    r.exact("embed LN1 weight", g[pe + "2.weight"], dgam); r.exact("embed LN1 bias", g[pe + "2.bias"], dbet)
    dp16 = r.S("dp16")
    r.exact("embed conv weight", g[pe + "0.weight"].reshape(pd, -1), dp16.T @ R.patchify(xn, r.patch).reshape(M, -1))
    r.exact("embed conv bias", g[pe + "0.bias"], dp16.sum(0))
    yst = r.S("yst")
    dycat, dgam, dbet = R.ln_bwd(r.S("dy"), r.S("ycat"), yst[:, :1], yst[:, 1:], w["norm.weight"])
    r.exact("cond LN backward dycat", r.S("dycat"), dycat)
    r.exact("norm.weight", g["norm.weight"], dgam); r.exact("norm.bias", g["norm.bias"], dbet)
    dycat = r.S("dycat")
    for tok in (0, 1):
        r.exact(f"cond LN backward token {tok}", dycat[tok::2], R.ln_bwd(r.S("dy"), r.S("ycat"), yst[:, :1], yst[:, 1:], w["norm.weight"])[0][tok::2])
    dnz, dlb = dycat[0::2], dycat[1::2]
    r.exact("label_proj weight", g["label_proj.weight"], dlb.T @ lab); r.exact("label_proj bias", g["label_proj.bias"], dlb.sum(0))
    r.exact("fourier_feats.3 weight", g["fourier_feats.3.weight"], dnz.T @ r.S("g1v")); r.exact("fourier_feats.3 bias", g["fourier_feats.3.bias"], dnz.sum(0))
    dg1 = (dnz @ w["fourier_feats.3.weight"]) * R.gelu_grad(r.S("h1"))
    r.exact("cond GELU backward dg1", r.S("dg1"), dg1)
    dg1 = r.S("dg1")
    r.exact("fourier_feats.1 weight", g["fourier_feats.1.weight"], dg1.T @ r.S("sinb")); r.exact("fourier_feats.1 bias", g["fourier_feats.1.bias"], dg1.sum(0))


def all_checks(r):
    forward_ends(r)
    for i in range(r.L):
        forward_block(r, i)
    for i in reversed(range(r.L)):
        backward_block(r, i)
    backward_ends(r)


# ---- tests ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=list(CASES))
def run(request):
    """Module-scoped, so pytest groups the tests by case: each engine is built once."""
    return run_case(request.param)


def test_forward_stages(run):
    r = run
    assert r.paths == r.expected_paths, f"case {r.name}: launch paths {r.paths:#x}, the plan predicts {r.expected_paths:#x}"
    n = len(r.rows); r.fail = []
    forward_ends(r)
    for i in range(r.L):
        forward_block(r, i)
    report(r, n)


def _backward(r):
    for i in reversed(range(r.L)):
        backward_block(r, i)
    backward_ends(r)
    r.backward_done = True


def test_backward_stages(run):
    r = run
    n = len(r.rows); r.fail = []
    _backward(r)
    report(r, n)


def test_every_parameter_gradient_is_checked_and_finite(run):
    """The backward stage checks read every parameter tensor of the engine's layout (none is exempted by its norm), and no gradient carries
    the poison."""
    r = run
    if not r.backward_done:
        _backward(r)
    missing = sorted(set(r.grads) - r.grads.read)
    assert not missing, f"case {r.name}: no stage check reads the gradient of {missing}"
    for k, v in r.grads.items():
        bad = int((~torch.isfinite(v)).sum())
        assert bad == 0, f"case {r.name} gradient {k}: {bad} of {v.numel()} values are NaN / Inf"
    assert bool(torch.isfinite(r.loss).all()) and bool(torch.isfinite(r.pred).all())


def _tn_off(case):
    code = ("import sys, json; sys.path.insert(0, %r); import test_gpu_train_stages as T; r = T.Run(%r)\n"
            "for i in reversed(range(r.L)): T.backward_block(r, i, weights_only=True)\n"
            "print('RESULT ' + json.dumps({'paths': r.paths, 'expected_paths': r.expected_paths, 'fail': r.fail, 'rows': [[a, b, c] for a, b, c, _ in r.rows]}))" % (os.path.join(REPO, "tests"), case))
    env = dict(os.environ, TLD_TRAIN_TN_WGRAD="0", PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=REPO, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


_TN_OFF = {}


@pytest.mark.parametrize("case", TN_OFF_CASES)
def test_transposing_weight_gradient_with_split_runs(case):
    """Case H: TLD_TRAIN_TN_WGRAD=0 in a fresh process -- every weight / bias / LayerNorm gradient of the blocks from its stage's own inputs."""
    res = _TN_OFF[case] = _tn_off(case)
    for a, b, c in res["rows"]:
        print(f"case {case} (TN off) {a:48s} {b:22s} {c:.3e}")
    assert not res["fail"], "\n".join(res["fail"])
    assert res["paths"] >> 26 & 1 and not res["paths"] >> 24 & 1, hex(res["paths"])
    assert res["paths"] == res["expected_paths"], f"case {case} (TN off): launch paths {res['paths']:#x}, the plan predicts {res['expected_paths']:#x}"


def test_cases_reach_every_launch_path():
    from transformer_latent_diffusion_amd import Trainer
    mask = 0
    for case in CASES:
        mask |= _PATHS[case] if case in _PATHS else run_case(case).paths
    for case in TN_OFF_CASES:
        mask |= (_TN_OFF[case] if case in _TN_OFF else _tn_off(case))["paths"]
    names = Trainer.PATH_NAMES
    # the one "masked" bit stands for several kernel pairs: split it by the dispatch's (mode, NW, masked) at each case's token count, hold the
    # three attention bits of every case against that, and require the instantiation of every product grid
    reached = set()
    for case, (kw, _, _) in CASES.items():
        n = (kw["image_size"] // kw["patch_size"]) ** 2
        mode, nw, masked = attn_bwd_dispatch(n)
        bits = _PATHS[case] >> names.index("attn_bwd_one_kernel") & 7
        assert bits == (1 if mode == "fused" else 2) | (4 if masked else 0), (case, n, bits, mode, nw, masked)
        reached.add((mode, nw, masked))
    unreached = sorted(n for n in GRIDS if attn_bwd_dispatch(n) not in reached)
    assert not unreached, f"product grids whose attention-backward instantiation no case runs: {unreached}"
    missing = [names[b] for b in range(len(names)) if not mask >> b & 1]
    print(f"launch paths reached: {bin(mask).count('1')} of {len(names)} (mask {mask:#x})")
    assert not missing, "launch paths no case reaches: " + ", ".join(missing)


def test_debug_calls_are_reproducible_and_debug_off_computes_the_same():
    """Case A: two debug calls on the same inputs give bitwise equal snapshots and gradients; a debug-off call gives bitwise the same gradient
    vector, loss and prediction."""
    r = run_case("A")
    names = ["blk1.gx.in", "blk1.dg", "blk1.dh", "blk1.gx.ln3", "blk1.dqc", "blk1.dkv", "blk1.dqkv", "blk0.gx.ln1", "blk1.gxb.ln1", "blk0.gl", "de", "dycat"]
    g1, l1, p1 = r.tr.grads.clone(), r.loss.clone(), r.pred.clone()
    first = {n: r.tr.read_stage(n) for n in names}
    loss2, pred2 = r.tr.forward_backward(*r.inputs)
    torch.cuda.synchronize()
    assert torch.equal(g1, r.tr.grads) and torch.equal(l1, loss2) and torch.equal(p1, pred2)
    for n in names:
        assert torch.equal(first[n].view(torch.int32), r.tr.read_stage(n).view(torch.int32)), n
    r.tr.set_debug(False)
    loss3, pred3 = r.tr.forward_backward(*r.inputs)
    torch.cuda.synchronize()
    same = torch.equal(g1, r.tr.grads) and torch.equal(l1, loss3) and torch.equal(p1, pred3)
    _RUN.pop("A", None)
    assert same

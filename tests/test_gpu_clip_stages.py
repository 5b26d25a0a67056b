"""GPU: the CLIP text tower (csrc/tld_clip.hip) stage by stage against float64, every row of every block, on the engine's own inputs.

tests/test_gpu_clip.py sees ``ln_final(x)[eot] @ text_projection`` only: one row per prompt, through a 2e-2 rel-rms.  Here every
transition of every block starts from the engine's snapshot of its inputs (tld_clip_set_debug; stage names in include/tld_hip.h and
DESIGN.md 7.9) and the operands as the engine holds them (bf16 projection weights read back through the hook; fp32 embeddings, biases and
LayerNorm affines, which ``upload_f32`` stores unchanged), is recomputed in float64 on the device with tests/clip_stage_refs.py (held
against the transformers fixture in tests/test_clip_stage_refs_host.py) and compared per element with the engine's snapshot of its
output.  Errors therefore do not pile up along the chain.  Every tensor is first checked for NaN / Inf (the hook fills the workspace with
0xFF bytes, so a kernel that stores nothing or too few rows shows as NaN).  Tolerance classes, none of them a new number:

* EXACT ``|got - ref| <= 2e-5 max|ref|`` (TAIL_TOL of tests/test_gpu_vae_blocks.py: fp32 arithmetic, only the order differs): x0, x1, x2,
  pooled, out;
* ROUND ``<= 2^-8 |ref| + 2e-5 sqrt(max(K, 64) / 64) max|ref|`` (the per-element form of tests/test_gpu_vae_blocks.py -- the exact fp32
  result rounded once to bf16 -- with the accumulation term of tests/test_gpu_gemm_epilogues.py; K is the length of the stage's longest
  fp32 sum): h1, h2 (K = W), qkv, f_pre (K = W), att (K = ctx; fp32 inside, rounded once), f (K = 64: elementwise, the fast reciprocal and
  exponential are fp32-ulp-sized);
* fp32 GEMM outputs ``<= 2e-5 max|A W^T| sqrt(K / 64) + 1e-5`` (the fp32-epilogue bound of tests/test_gpu_gemm_epilogues.py): attn_out
  (K = W), mlp_out (K = 4 W).

Besides the whole tensor, the worst value / bound is reported and held for: the first and the last row; rows at position i < 64, i = 64,
i > 64 of their prompt (the second key per lane of clip_attn_kernel goes live at 64); the last T mod 4 rows (the partial group of the
one-wave-per-row kernels); the rows after each prompt's EOT (which reach no output); each (prompt, head) -- each (prompt, 64-column group)
of the wider stages; the last 64-column lane slot.  With TLD_CLIP_STAGE_RECORD=<file> a summary per case is appended to that file;
profiles/r12_clip_stage_errors.txt is such a run.

Cases (CASES below): the true ViT-L/14 geometry at the shipped batch of 64 prompts (T = 4928: 360 in_proj tiles on 256 CUs with two XCD
groups, c_fc on 256-wide ring tiles, a ragged last row tile) and at 37 (odd T); ctx = 128 (the largest dynamic LDS request, 99 328 bytes
of the part's 160 KiB per workgroup), 64 and 65 (the second key per lane), width 1024 (all 16 register slots of the row kernels) and 64
(one head, one element per lane, K = 64), and the chunked tiny case.  Every case has a prompt with its EOT at position 1, one at ctx - 1
and, where ctx allows, one at >= 64.  test_cases_reach_the_gemm_plans (CPU) holds the launch plans the cases are there for.

The tests bite (profiles/r12_clip_stage_mutations.txt): six numeric, in-bounds mutations of tld_clip.hip, one library each, run once
against this file and against tests/test_gpu_clip.py.  Value / bound of the first failing stage, worst case:
  the score phase admits key i + 1 (one-position causal leak): att 254 in all 7 cases, both causality tests fail; test_gpu_clip.py 4 of 7 fail;
  the P.V loop drops the diagonal key for rows i >= 64: att 24 (CTX65) ... 3.5e3 (L14), cases L14 / CTX128 / CTX65; test_gpu_clip.py fails only
    its two ViT-L/14 tests;
  QuickGELU's 1.702 becomes 1.7: f 1.43 ... 1.55 in all 7 cases; test_gpu_clip.py PASSES;
  clip_add_ln_kernel skips the bias in the last lane slot: x1 451 ... 989 in all 7 cases; test_gpu_clip.py 4 fail (rel-rms 3.1e-2);
  clip_final_ln_kernel takes mean / rstd from the row before the add: pooled 2.6e3 ... 1.1e4 in all 7 cases; test_gpu_clip.py fails only its two
    tiny tests;
  clip_embed_kernel reads pos[i - 1] at positions i >= 64: x0 2.4e4 ... 2.9e4, cases L14 / CTX128 / CTX65; test_gpu_clip.py fails only its two
    ViT-L/14 tests.
Found by this file: nothing -- every comparison on the unmutated library is within its bound (worst value / bound 0.984, the bf16 rounding itself;
EXACT <= 0.008, fp32 GEMM outputs <= 0.007), including ctx = 128, which had never been launched.
Wall time on an MI355X: the file 5 s; L14 2.4 s (weights for a 49 408-row embedding and 64 prompts), every other case below 0.6 s.
"""
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import clip_stage_refs as R
from test_clip_host import TINY, _tokens
from test_gemm_plan import BN, EPI_BIAS_BF16, EPI_F32, FAMILY, MAIN, RING, XCD, plan
from test_gpu_parity import _dev
from transformer_latent_diffusion_amd.clip_text import ClipTextConfig

gpu = pytest.mark.gpu

TLD_ERR_KEY, TLD_ERR_SHAPE = 2, 3            # include/tld_hip.h
EXACT_TOL = 2e-5                             # TAIL_TOL, tests/test_gpu_vae_blocks.py
ROUND_REL = 2.0 ** -8                        # half a bf16 ulp, relative (tests/test_gpu_vae_blocks.py)
ACC_TOL = 2e-5                               # fp32 accumulation per sqrt(K / 64), tests/test_gpu_gemm_epilogues.py
GEMM32_ABS = 1e-5                            # ... and its absolute term


def _small(ctx, width, layers):
    return ClipTextConfig(vocab_size=1000, context_length=ctx, width=width, heads=width // 64, layers=layers, embed_dim=64)


# name: (config, max_batch, batches run one after the other on one engine, weight seed)
CASES = {
    "L14": (ClipTextConfig(layers=2), 64, (64, 37), 0),
    "CTX128": (_small(128, 128, 2), 3, (3,), 1),
    "CTX64": (_small(64, 128, 2), 3, (3,), 2),
    "CTX65": (_small(65, 128, 2), 3, (3,), 3),
    "W1024": (_small(16, 1024, 2), 3, (3,), 4),
    "W64": (_small(16, 64, 3), 5, (5,), 5),
    "TINY": (TINY, 4, (11,), 6),
}
assert CASES["TINY"][0] == _small(16, 128, 2)


def _chunks(B, max_batch):
    return [(b0, min(B, b0 + max_batch)) for b0 in range(0, B, max_batch)]


def _prompts(cfg, B, max_batch, seed):
    """_tokens, with the EOT of the first prompts of the LAST chunk (the one the stages hold) moved to position 1, ctx - 1 and >= 64."""
    t = _tokens(cfg, B, seed)
    g = torch.Generator().manual_seed(seed + 977)
    ctx, V = cfg.context_length, cfg.vocab_size
    b0, b1 = _chunks(B, max_batch)[-1]
    wanted = [1, ctx - 1] + ([64 + (ctx - 65) // 2] if ctx > 64 else [])
    assert b1 - b0 >= len(wanted)
    for b, e in zip(range(b0, b1), wanted):
        t[b] = 0
        t[b, 0] = V - 2
        if e > 1:
            t[b, 1:e] = torch.randint(1, V - 2, (e - 1,), generator=g)
        t[b, e] = V - 1
    eot = t.argmax(dim=-1)
    assert sorted(set(wanted)) == sorted(set(eot[b0:b0 + len(wanted)].tolist()))
    return t


def _encoder(cfg, max_batch, seed):
    from transformer_latent_diffusion_amd.clip_text import ClipTextEncoder, synth_clip_state_dict
    sd = synth_clip_state_dict(cfg, seed)
    enc = ClipTextEncoder(cfg, max_batch=max_batch)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return sd, enc.to(_dev())


def _stage_names(cfg):
    names = ["x0"]
    for i in range(cfg.layers):
        names += [f"blk{i}.{s}" for s in ("h1", "qkv", "att", "attn_out", "x1", "h2", "f_pre", "f", "mlp_out")]
        if i + 1 < cfg.layers:
            names.append(f"blk{i}.x2")
    return names + ["pooled", "out"]


def _record(line):
    path = os.environ.get("TLD_CLIP_STAGE_RECORD")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


class Checks:
    """Per-element comparisons of one encode: worst |got - ref| / bound of the whole tensor and of every row / column class."""

    def __init__(self, name, cfg, batch, eot):
        self.name, self.fail, self.rows = name, [], []          # rows: (stage, tolerance class, row class, worst ratio)
        ctx = cfg.context_length
        T, dev = batch * ctx, eot.device
        self.batch, self.ctx = batch, ctx
        pos = torch.arange(T, device=dev) % ctx
        after = pos > eot.long().repeat_interleave(ctx)
        idx = torch.arange(T, device=dev)
        masks = {"first row": idx == 0, "last row": idx == T - 1, "rows i < 64": pos < 64, "rows i = 64": pos == 64, "rows i > 64": pos > 64,
                 "last T mod 4 rows": idx >= T - T % 4, "rows after EOT": after}
        self.masks = {k: m for k, m in masks.items() if bool(m.any())}

    def _note(self, stage, tol, cls, val):
        self.rows.append((stage, tol, cls, val))
        if not val <= 1.0:
            self.fail.append(f"{self.name} {stage} [{tol}] {cls}: value / bound = {val:.3g}")

    def compare(self, stage, tol, got, ref, bound):
        """got fp32, ref float64, bound float64 per element (same shape)."""
        bad = int((~torch.isfinite(got)).sum())
        if bad:
            self.fail.append(f"{self.name} {stage}: {bad} of {got.numel()} values are NaN / Inf")
            self.rows.append((stage, tol, "finite", float("inf")))
            print(f"{self.name:7s} {stage:14s} {tol:6s} {bad} of {got.numel()} values are NaN / Inf")
            return
        assert got.shape == ref.shape, (stage, got.shape, ref.shape)
        ratio = (got.double() - ref).abs() / bound
        rows, cols = ratio.shape
        rowmax = ratio.amax(dim=1)
        vals = {"whole": rowmax.max()}
        if rows == self.batch * self.ctx:
            for k, m in self.masks.items():
                vals[k] = rowmax[m].max()
            per = ratio.view(self.batch, self.ctx, cols // 64, 64).amax(dim=(1, 3))
        else:                                                    # pooled, out: one row per prompt
            per = ratio.view(self.batch, 1, cols // 64, 64).amax(dim=(1, 3))
        vals["worst (prompt, 64 columns)"] = per.max()
        vals["last lane slot"] = ratio[:, -64:].max()
        host = torch.stack(list(vals.values())).cpu().tolist()
        where = int(per.argmax())
        for k, v in zip(vals, host):
            self._note(stage, tol, k, v)
        print(f"{self.name:7s} {stage:14s} {tol:6s} " + "  ".join(f"{k} {v:.3f}" for k, v in zip(vals, host)) +
              f"  (prompt {where // per.shape[1]}, group {where % per.shape[1]})  max|err| {float((got.double() - ref).abs().max()):.3e}")

    def exact(self, stage, got, ref):
        self.compare(stage, "EXACT", got, ref, torch.full_like(ref, EXACT_TOL * float(ref.abs().max())))

    def round(self, stage, got, ref, K):
        self.compare(stage, "ROUND", got, ref, ROUND_REL * ref.abs() + ACC_TOL * (max(K, 64) / 64) ** 0.5 * float(ref.abs().max()))

    def gemm32(self, stage, got, ref, K):
        self.compare(stage, "GEMM32", got, ref, torch.full_like(ref, ACC_TOL * float(ref.abs().max()) * (K / 64) ** 0.5 + GEMM32_ABS))

    def summary(self):
        worst = {}
        for stage, tol, cls, v in self.rows:
            for key in (("tolerance", tol), ("rows", cls)):
                if key not in worst or not v <= worst[key][0]:
                    worst[key] = (v, stage)
        return [f"  {kind:9s} {k:28s} worst value / bound {v:.3f}  ({stage})" for (kind, k), (v, stage) in sorted(worst.items(), key=lambda kv: kv[0][0] != "tolerance")]


def _check_encode(name, cfg, sd, enc, tokens, out):
    """Every transition of every block of the LAST chunk of this encode."""
    dev = _dev()
    b0, b1 = _chunks(tokens.shape[0], enc.max_batch)[-1]
    tok = tokens[b0:b1].to(dev)
    B, ctx, W, L = b1 - b0, cfg.context_length, cfg.width, cfg.layers
    eot = tok.argmax(dim=-1)
    c = Checks(f"{name}/{tokens.shape[0]}", cfg, B, eot)
    st = lambda n: enc.read_stage(n).to(dev)
    w32 = lambda k: torch.from_numpy(sd[k]).to(dev)             # fp32 operands: uploaded unchanged
    blk = lambda i, k: w32(f"transformer.resblocks.{i}.{k}")

    x = st("x0")
    assert x.shape == (B * ctx, W)
    c.exact("x0", x, R.embed(tok, w32("token_embedding.weight"), w32("positional_embedding")))
    h = st("blk0.h1")
    c.round("blk0.h1", h, R.add_layer_norm(x, None, None, blk(0, "ln_1.weight"), blk(0, "ln_1.bias"))[1], W)
    for i in range(L):
        p = f"blk{i}."
        qkv = st(p + "qkv")
        c.round(p + "qkv", qkv, R.in_proj(h, st(p + "in_w"), blk(i, "attn.in_proj_bias")), W)
        att = st(p + "att")
        c.round(p + "att", att, R.causal_attention(qkv, B, ctx), ctx)
        del qkv
        ao = st(p + "attn_out")
        c.gemm32(p + "attn_out", ao, R.out_proj(att, st(p + "out_w")), W)
        x1, h2 = st(p + "x1"), st(p + "h2")
        rx, _ = R.add_layer_norm(x, ao, blk(i, "attn.out_proj.bias"), blk(i, "ln_2.weight"), blk(i, "ln_2.bias"))
        c.exact(p + "x1", x1, rx)
        c.round(p + "h2", h2, R.layer_norm(x1, blk(i, "ln_2.weight"), blk(i, "ln_2.bias")), W)
        del att, ao, rx
        f_pre = st(p + "f_pre")
        c.round(p + "f_pre", f_pre, R.c_fc(h2, st(p + "fc_w"), blk(i, "mlp.c_fc.bias")), W)
        f = st(p + "f")
        c.round(p + "f", f, R.quick_gelu(f_pre), 64)
        del f_pre
        mo = st(p + "mlp_out")
        c.gemm32(p + "mlp_out", mo, R.c_proj(f, st(p + "proj_w")), 4 * W)
        del f
        if i + 1 < L:
            x, h = st(p + "x2"), st(f"blk{i + 1}.h1")
            c.exact(p + "x2", x, x1.double() + mo.double() + blk(i, "mlp.c_proj.bias").double())
            c.round(f"blk{i + 1}.h1", h, R.layer_norm(x, blk(i + 1, "ln_1.weight"), blk(i + 1, "ln_1.bias")), W)
        else:
            pooled = st("pooled")
            c.exact("pooled", pooled, R.final_add_layer_norm(x1, mo, blk(i, "mlp.c_proj.bias"), eot, w32("ln_final.weight"), w32("ln_final.bias"), ctx))
            got = st("out")
            c.exact("out", got, R.projection(pooled, st("proj_t")))
            assert torch.equal(got, out[b0:b1]), "the 'out' stage is not what encode_text returned"
    return c


def _run_case(name):
    cfg, max_batch, batches, seed = CASES[name]
    t0 = time.time()
    sd, enc = _encoder(cfg, max_batch, seed)
    enc.set_debug(True)
    fails, lines = [], []
    for B in batches:
        tokens = _prompts(cfg, B, max_batch, seed + B)
        out = enc.encode_text(tokens.to(_dev()))
        torch.cuda.synchronize()
        c = _check_encode(name, cfg, sd, enc, tokens, out)
        fails += c.fail
        lines += [f"{c.name}: ctx {cfg.context_length} width {cfg.width} layers {cfg.layers} max_batch {max_batch}, {len(c.rows)} bounded values, "
                  f"{len(c.fail)} above their bound"] + c.summary()
    enc.set_debug(False)
    enc._drop_engine()
    lines.append(f"{name}: {time.time() - t0:.1f} s")
    print("\n".join(lines))
    for ln in lines:
        _record(ln)
    return fails


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_every_stage_of_every_block(name):
    fails = _run_case(name)
    assert not fails, "\n".join(fails[:40])


# ---- causality, bitwise -------------------------------------------------------------------------------------------------------

def _all_stages(enc, cfg):
    return {n: enc.read_stage(n) for n in _stage_names(cfg)}


@gpu
@pytest.mark.parametrize("name,p", [("CTX65", 63), ("TINY", 7)])
def test_rows_do_not_see_later_tokens(name, p):
    """Other ids after position p: every stage row at a position <= p of every block, and out of the prompts whose EOT is <= p, keep their bits
    (p = 63 at ctx 65: row 63 must not see key 64, the first one of the second lane half)."""
    cfg, max_batch, batches, seed = CASES[name]
    sd, enc = _encoder(cfg, max_batch, seed)
    enc.set_debug(True)
    B = batches[-1]
    tokens = _prompts(cfg, B, max_batch, seed + B)
    out_a = enc.encode_text(tokens.to(_dev())).cpu()
    a = _all_stages(enc, cfg)
    other = tokens.clone()
    g = torch.Generator().manual_seed(seed)
    other[:, p + 1:] = torch.randint(1, cfg.vocab_size - 2, other[:, p + 1:].shape, generator=g)
    assert not torch.equal(other, tokens)
    out_b = enc.encode_text(other.to(_dev())).cpu()
    b = _all_stages(enc, cfg)
    eot = tokens.argmax(dim=-1)
    early = eot <= p
    assert bool(early.any()) and bool((~early).any())
    assert torch.equal(out_a[early], out_b[early])
    assert not torch.equal(out_a[~early], out_b[~early])                              # (the change does reach the later rows)
    b0, b1 = _chunks(B, max_batch)[-1]
    ctx = cfg.context_length
    keep = (torch.arange((b1 - b0) * ctx) % ctx) <= p
    for n in _stage_names(cfg):
        assert bool(torch.isfinite(a[n]).all()) and bool(torch.isfinite(b[n]).all()), n
        if n in ("pooled", "out"):
            assert torch.equal(a[n][early[b0:b1]], b[n][early[b0:b1]]), n
        else:
            assert torch.equal(a[n][keep], b[n][keep]), f"{n}: rows at positions <= {p} changed with the ids after {p}"
            assert n == "x0" or p + 1 >= ctx or not torch.equal(a[n][~keep], b[n][~keep]), n
    enc._drop_engine()


# ---- the clamps, through the C ABI --------------------------------------------------------------------------------------------

@gpu
def test_out_of_range_ids_and_eot_are_clamped():
    """Token ids -3 and vocab + 9, EOT -1 and ctx + 5 give bitwise the result of 0, vocab - 1, 0 and ctx - 1 (clip_embed_kernel, clip_final_ln_kernel)."""
    from transformer_latent_diffusion_amd import _lib
    cfg, max_batch, _, seed = CASES["TINY"]
    sd, enc = _encoder(cfg, max_batch, seed)
    dev = _dev()
    enc._ensure_engine(dev)
    enc.set_debug(True)
    L, V, ctx = _lib.lib(), cfg.vocab_size, cfg.context_length
    tok = _tokens(cfg, 3, 9).to(torch.int32)
    raw, clamped = tok.clone(), tok.clone()
    for (b, i), (bad, good) in {(0, 2): (-3, 0), (1, 0): (V + 9, V - 1), (2, ctx - 1): (-3, 0), (2, 5): (V + 9, V - 1)}.items():
        raw[b, i], clamped[b, i] = bad, good
    eots = {"raw": torch.tensor([-1, ctx + 5, 3], dtype=torch.int32), "clamped": torch.tensor([0, ctx - 1, 3], dtype=torch.int32)}
    res = {}
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for key, t in (("raw", raw), ("clamped", clamped)):
        td, ed = t.to(dev).contiguous(), eots[key].to(dev)
        out = torch.full((3, cfg.embed_dim), float("nan"), device=dev)
        _lib.check(L.tld_clip_encode_text(enc._engine, C.c_void_p(td.data_ptr()), C.c_void_p(ed.data_ptr()), C.c_void_p(out.data_ptr()), 3, st), key)
        torch.cuda.synchronize()
        res[key] = dict(_all_stages(enc, cfg), returned=out.cpu())
    for n, v in res["raw"].items():
        assert bool(torch.isfinite(v).all()), n
        assert torch.equal(v, res["clamped"][n]), n
    enc._drop_engine()


# ---- the hook itself ----------------------------------------------------------------------------------------------------------

@gpu
def test_the_hook_changes_nothing_and_refuses_what_it_does_not_have():
    from transformer_latent_diffusion_amd import _lib
    cfg, max_batch, _, seed = CASES["TINY"]
    sd, enc = _encoder(cfg, max_batch, seed)
    tokens = _prompts(cfg, 3, max_batch, 12).to(_dev())
    off = enc.encode_text(tokens).clone()
    L = _lib.lib()
    buf = np.empty(3 * cfg.context_length * cfg.width, np.float32)
    ptr, name = buf.ctypes.data_as(C.POINTER(C.c_float)), b"blk0.h1"
    assert L.tld_clip_read_stage(enc._engine, name, ptr, buf.size, None) == TLD_ERR_KEY            # debug off: nothing is kept
    enc.set_debug(True)
    on1 = enc.encode_text(tokens).clone()
    first = _all_stages(enc, cfg)
    on2 = enc.encode_text(tokens).clone()
    for n, v in first.items():
        assert bool(torch.isfinite(v).all()) and torch.equal(v, enc.read_stage(n)), n               # deterministic stage by stage
    shape = (C.c_int64 * 4)()
    assert L.tld_clip_read_stage(enc._engine, name, ptr, buf.size, shape) == 0 and list(shape) == [3 * cfg.context_length, cfg.width, 1, 1]
    assert L.tld_clip_read_stage(enc._engine, name, ptr, buf.size - 1, shape) == TLD_ERR_SHAPE
    assert L.tld_clip_read_stage(enc._engine, b"blk0.nonsense", ptr, buf.size, shape) == TLD_ERR_KEY
    assert L.tld_clip_read_stage(enc._engine, b"blk7.h1", ptr, buf.size, shape) == TLD_ERR_KEY
    assert L.tld_clip_read_stage(enc._engine, b"blk7.in_w", ptr, buf.size, shape) == TLD_ERR_KEY
    last = cfg.layers - 1
    assert L.tld_clip_read_stage(enc._engine, f"blk{last}.x2".encode(), ptr, buf.size, shape) == TLD_ERR_KEY and b"no captured stage" in L.tld_last_error()
    assert L.tld_clip_read_stage(enc._engine, b"blk0.x2", ptr, buf.size, shape) == 0
    with pytest.raises(RuntimeError, match="no captured stage"):
        enc.read_stage(f"blk{last}.x2")
    enc.set_debug(False)
    assert L.tld_clip_read_stage(enc._engine, name, ptr, buf.size, shape) == TLD_ERR_KEY            # snapshot memory is gone
    assert enc.read_stage("blk0.in_w").shape == (3 * cfg.width, cfg.width)                           # operands are read in place: no debug call needed
    off2 = enc.encode_text(tokens).clone()
    assert torch.equal(off, on1) and torch.equal(on1, on2) and torch.equal(off, off2)
    enc._drop_engine()


# ---- CPU: the launch plans the cases are there for -----------------------------------------------------------------------------

def _projection_plans(name):
    cfg, max_batch, batches, _ = CASES[name]
    W = cfg.width
    for B in batches:
        for b0, b1 in _chunks(B, max_batch):
            M = (b1 - b0) * cfg.context_length
            for what, (N, K, epi) in dict(in_proj=(3 * W, W, EPI_BIAS_BF16), out_proj=(W, W, EPI_F32), c_fc=(4 * W, W, EPI_BIAS_BF16),
                                          c_proj=(W, 4 * W, EPI_F32)).items():
                yield what, M, N, K, plan(M, N, K, epi, ncu=256)


def test_cases_reach_the_gemm_plans():
    """plan_gemm (tests/test_gemm_plan.py) at 256 CUs on the four projections of every case: together they reach what tests/test_gpu_clip.py's batches do not."""
    seen = {k: [] for k in ("128-wide two-stage", "256-wide ring", "xcd_ngroups 2", "more tiles than CUs", "ragged last row tile", "K = 64")}
    for name in CASES:
        for what, M, N, K, p in _projection_plans(name):
            assert p[FAMILY] == MAIN, (name, what, M, N, K, p)
            tiles = -(-M // 256) * -(-N // int(p[BN]))
            tag = f"{name} {what} M {M}"
            if p[BN] == 128 and p[RING] == 0:
                seen["128-wide two-stage"].append(tag)
            if p[BN] == 256 and p[RING] == 1:
                seen["256-wide ring"].append(tag)
            if p[XCD] == 2:
                seen["xcd_ngroups 2"].append(tag)
            if tiles > 256:
                seen["more tiles than CUs"].append(tag)
            if M > 256 and M % 256:
                seen["ragged last row tile"].append(tag)
            if K == 64:
                seen["K = 64"].append(tag)
    for k, v in seen.items():
        assert v, f"no case reaches: {k}"
    # the shipped call: 64 prompts at ViT-L/14 width
    l14 = {(what, M): (N, K, p) for what, M, N, K, p in _projection_plans("L14")}
    N, K, p = l14[("in_proj", 4928)]
    assert (p[BN], p[RING], p[XCD]) == (128, 0, 2) and 20 * (N // 128) == 360
    N, K, p = l14[("c_fc", 4928)]
    assert (p[BN], p[RING]) == (256, 1)
    assert 4928 % 256 == 64
    # ... and none of tests/test_gpu_clip.py's ViT-L/14 batches (4 and 8 prompts) leaves the 128-wide two-stage tiles or fills the chip
    for B in (4, 8):
        for N, K, epi in ((2304, 768, EPI_BIAS_BF16), (768, 768, EPI_F32), (3072, 768, EPI_BIAS_BF16), (768, 3072, EPI_F32)):
            p = plan(B * 77, N, K, epi, ncu=256)
            assert (p[BN], p[RING], p[XCD]) == (128, 0, 0) and -(-B * 77 // 256) * (N // 128) < 256

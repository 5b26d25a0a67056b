"""GPU: the inference forward at every token grid the engine accepts, class by class against float64.

tld_engine_create takes any square token grid whose side G is a multiple of 4.  What a forward launches depends on G (tests/test_forward_grids_host.py
restates the dispatch and holds the case tables of this file against it on the host); this file runs every grid up to 64 x 64 tokens through the two
grid-dependent hooks alone and through the engine, with the machinery and the tolerance classes of tests/test_gpu_forward_stages.py (Checks,
run_forward_case, _sampler; EXACT 2e-5 max|ref|, ROUND 2^-8 |ref| + 2e-5 sqrt(max(K, 64) / 64) max|ref|, MODELLED at twice the float64 rounding model's
own error, member by member of every class) and of tests/test_gpu_fp8_stages.py.  No tolerance is introduced here.

a. test_depthwise_hook: tld_debug_dwconv_gelu at G = 4, 8 ... 64 and 96 (three strips), 64 and 128 channels, batch 3 up to G = 40 and 2 above, against
   float64 train_stage_refs.dwconv_fwd + the exact GELU of the same bf16 inputs.  Whole-image kernel (G <= 16): ROUND, every element.  Tiled and
   streaming kernels: MODELLED with infer_stage_refs.dw_gelu_model -- whole tensor, each sample, each 64-channel slab, corner / edge / interior
   pixels, and per kernel the classes of test_forward_grids_host.pixel_classes: the 16 x 16 tile seams, the pixels of the partial last tiles, their
   outermost column and lowest row; the strip-seam columns; (whole image: the last G % 3 columns of the column rotation, held by ROUND like every
   element).  The output starts as NaN, a guard band of one image row behind the last row is compared bitwise, two runs are bitwise equal.
b. test_attention_hook: tld_debug_attention_fwd at N = 16 k^2, k = 1 ... 16, (samples, heads) = (3, 2) up to 1600 tokens and (1, 2) above, against
   float64 exact attention, MODELLED with infer_stage_refs.attn_model: whole tensor, each sample, each (sample, head), first and last row, and for
   the masked kernel the rows of the last partial 128-query block and its first 32-row wave, per (sample, head).  Families: random; rising scores;
   every score strongly negative / positive (-300 ... -150 and 150 ... 300 log2 units); and two tail-peaked families in which one key holds most of
   every query's weight -- key N - 1, next to the mask, and key N - N % 128, the first of the partial chunk (masked counts only): the host file
   shows that dropping either key moves every class by more than ten yardsticks.  NaN pre-fill, guard rows, run-to-run identity as in (a).
c. test_engine_stages: one forward of a two-block engine at every G = 4 ... 64, stage by stage, in three families: d = 256 bf16 (MFMA cross_row,
   LayerNorm q4, the LayerNorm-3 fold, embed_mfma, tail_mfma), d = 192 bf16 (VALU cross_row, generic LayerNorm, plain embed and tail), and d = 256
   MX-fp8 at G = 4, 12, 20, 28, 36, 44 (unfused and fused engines: the whole-image kernel with the separate quantisation pass, the tiled fp8 writer
   at remainders 4 and 12).  Neither width takes the LayerNorm-1 fold (test_forward_grids_host.fold_ln1: of the widths in use only d = 768
   does), so that fold is not swept over the grids here: it is row-local, its one grid-dependent consumer is the fused QKV + attention at 256
   tokens, and tests/test_gpu_forward_stages.py holds both at d = 768.  GridChecks adds the pixel classes of (a) to every MODELLED depthwise
   transition and the partial-query-block classes of (b) to every self-attention.  test_cross_row_partition:
   (G, batch) = (8, 128), (24, 29), (24, 15) at d = 256 -- on 256 CUs gpw 2 with four groups per sample, gpw 4 and gpw 2 with 36; the expected gpw comes from the device's CU count by launch_cross_row's rule and is the one the
   workgroup-boundary class uses.  test_sampler_grids: DPM-Solver++, three steps, CFG with layer-0 sharing, at G = 12, 20, 28, every step's stages.
   Every case asserts its tld_engine_debug_paths mask bit by bit against test_forward_grids_host.expected_paths: attention form, depthwise form
   and its fp8 writer, cross_row form and gpw bit, the up-projection fused or alone, the x_in fan-out.

With TLD_FORWARD_GRID_RECORD=<file> every case appends its summary to that file in the format of TLD_FORWARD_STAGE_RECORD:
profiles/forward_grid_errors.txt is such a run.

Found by this file: nothing -- on an MI355X all 169 tests pass on the unmutated library, and no kernel is changed.  Measured = yardstick to two or
three digits in every class of more than one row; worst EXACT 3.2e-6 of 2e-5, worst ROUND 0.99 of its bound.  Of 2796 MODELLED class figures 22 lie
more than 1.2 x above their yardstick, all single rows of 64 ... 256 values (first / last query per (sample, head), first / last row); the worst is
1.69 x (the chunked kernel at 1024 tokens, rising scores, first query: 2.90e-3 against 1.72e-3), inside the bound of 2 x.

The checks bite (profiles/forward_grid_mutations.txt): five numeric, in-bounds mutations, each confined to one class of grids, one library each
(TLD_LIB).  Each library ran once on an MI355X -- this file, then the older forward tests ("old": tests/test_gpu_forward_stages.py,
test_gpu_fp8_stages.py, test_gpu_attention.py, test_gpu_dwconv.py, test_gpu_fp8.py, test_gpu_configs.py's sampler on unspecialised grids,
test_gpu_parity.py's forward vs golden; 108 tests).  Every mutation fails here; 1 and 5 pass every older test.
  1 tiled depthwise, G % 16 == 4: the right zero-padding column of the partial tile reads the halo's clamped copy: 15 fail here, every case at grids
    20, 36, 52 (depthwise MODELLED 16.9 ... 371 x the bound, a8_down 1.21 ... 13 x); old: all 108 pass
  2 tiled depthwise, fp8 writer: the scale byte of the partial tile's last column taken from its left neighbour: 4 fail here (fp8 at g20, g28, g36, g44:
    the fused engine's a8_down scale bytes differ bitwise from the separate pass, MODELLED 1.23 ... 21.5 x); old: 4 of test_gpu_fp8_stages.py fail
    (remainder 8: T24, T40, W640, T24s), remainders 4 and 12 only here
  3 whole-image depthwise, G % 3 == 1: the final emit uses the left column twice: 7 fail here (the hook at G = 4 and 16, the three engines at G = 4;
    ROUND 7.1e+3 ... 1.6e+4 x, the "last column of the rotation" class of a8_down 13.6 x); old: 5 fail, all at G = 16; G = 4 only here
  4 masked attention, N % 128 == 16: the key limit 8 keys too high: 61 fail here -- the hook at every N = 16 k^2 with k odd (peak last 191 ... 1460 x
    in every class, the other families 1.03 ... 288 x), every engine and sampler case at G = 4, 12 ... 60; nothing at N % 128 == 64 or 0.  Old: 11 fail
    (test_gpu_attention.py at 16, 144, 400, 1296, 3600, the sampler at 12 x 12 and 20 x 20); the stage files pass
  5 cross_row_mfma_kernel, group count no power of two: the last group of a workgroup takes the previous group's LN3 statistics: 2 fail here
    (test_cross_row_partition[24-29] and [24-15], 36 groups at gpw 4 and 2: LN3 mean 1.0 and 1.2, LN3 rstd 2.7e-1 and 2.4e-1 against EXACT 2e-5; [8-128],
    four groups, passes as it must); old: all 108 pass

Wall time on an MI355X: 14 s for this file run alone (169 tests, none above 0.7 s).
"""
import ctypes as C
import gc
import os

import numpy as np
import pytest
import torch

import infer_stage_refs as F
import test_forward_grids_host as HG
import test_gpu_forward_stages as FS
import test_gpu_fp8_stages as F8
from test_gpu_parity import _dev

pytestmark = pytest.mark.gpu

NAN_BITS = 0x7FC0            # torch's bf16 NaN: the pre-fill of every output and guard band
_PATHS = {}


def _cus():
    return torch.cuda.get_device_properties(_dev()).multi_processor_count


def _recorded(fn):
    """Run fn with the stage file's record switch pointing at this file's."""
    path = os.environ.get("TLD_FORWARD_GRID_RECORD")
    return FS._with_env({"TLD_FORWARD_STAGE_RECORD": path}, fn) if path else fn()


def _rel(es, rs, whole):
    """Checks.classes' figure: the relative rms of every member; a member whose reference is (numerically) zero is held to the whole tensor's size."""
    es, rs = es.reshape(-1), rs.reshape(-1)
    ok = rs > 1e-6 * whole / max(rs.numel(), 1)
    return torch.where(ok, es / rs.clamp_min(1e-300), es / (whole / max(rs.numel(), 1))).sqrt()


class GridChecks(FS.Checks):
    """The stage file's classes, and per grid: the pixel classes of the depthwise kernel the grid takes (pixels) and the masked attention kernel's
    partial query block, per (sample, head) (heads).  slabs: each 64-channel slab (the hook tests)."""
    slabs = False
    expect_gpw = None

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        assert self.expect_gpw is None or self.gpw == self.expect_gpw, f"{self.name}: gpw {self.gpw} from the device, {self.expect_gpw} restated"

    def classes(self, got, ref, samples, heads, pixels):
        out = super().classes(got, ref, samples, heads, pixels)
        N, H = self.N, self.H
        e2, r2 = (got - ref) ** 2, ref ** 2
        F_ = e2.shape[-1]
        whole = float(r2.sum())
        e3, r3 = e2.view(samples, N, F_), r2.view(samples, N, F_)
        if pixels:
            for tag, m in HG.pixel_classes(self.G).items():
                if tag not in out:
                    m = m.reshape(-1).to(e2.device)
                    out[tag] = _rel(e3[:, m].sum(), r3[:, m].sum(), whole)
        if heads:
            for tag, m in HG.query_classes(N).items():
                m = m.to(e2.device)
                out[tag] = _rel(e3[:, m].reshape(samples, -1, H, F_ // H).sum((1, 3)), r3[:, m].reshape(samples, -1, H, F_ // H).sum((1, 3)), whole)
        if self.slabs:
            out["64-channel slab"] = _rel(e3.view(samples, N, F_ // 64, 64).sum((0, 1, 3)), r3.view(samples, N, F_ // 64, 64).sum((0, 1, 3)), whole)
        return out


class HookChecks(GridChecks):
    slabs = True


class GridChecks8(GridChecks, F8.Checks8):
    pass


def _with_gpw(base, gpw):
    return type(base.__name__, (base,), {"expect_gpw": gpw})


def _guarded(rows, width, guard_rows):
    """A bf16 NaN buffer of rows + guard_rows rows: (whole buffer, the rows, the guard band as int16)."""
    buf = torch.full(((rows + guard_rows) * width,), float("nan"), dtype=torch.bfloat16, device=_dev())
    return buf, buf[:rows * width].view(rows, width), buf[rows * width:].view(torch.int16)


def _check_guard(c, guard):
    want = torch.full_like(guard, NAN_BITS).double()
    c.equal("guard band behind the last row (bitwise)", guard.double(), want)


# ---- a. the depthwise hook alone -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,batch,ch", HG.DW_HOOK)
def test_depthwise_hook(G, batch, ch):
    from transformer_latent_diffusion_amd import _lib
    dev, N = _dev(), G * G
    gen = torch.Generator().manual_seed(900 + 7 * G + ch)
    x = torch.randn(batch, N, ch, generator=gen).bfloat16()
    w = (torch.randn(ch, 9, generator=gen) * 0.4).float()
    b = (torch.randn(ch, generator=gen) * 0.2).float()
    wf, bf = np.ascontiguousarray(w.numpy()), np.ascontiguousarray(b.numpy())
    xd = x.to(dev)

    def run():
        buf, out, guard = _guarded(batch * N, ch, G)
        _lib.check(_lib.lib().tld_debug_dwconv_gelu(xd.data_ptr(), wf.ctypes.data_as(C.POINTER(C.c_float)), bf.ctypes.data_as(C.POINTER(C.c_float)),
                                                    buf.data_ptr(), batch, G, ch, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tld_debug_dwconv_gelu")
        torch.cuda.synchronize()
        return out, guard
    out, guard = run()
    form, rem = HG.depthwise_class(G)
    c = HookChecks(f"dw{G}x{ch}", batch, N, G, 1)
    got = out.double()
    x64, w64, b64 = xd.double(), w.to(dev).double(), b.to(dev).double()
    exact = F.dw_gelu(x64, w64, b64, G).reshape(batch * N, ch)
    what = f"depthwise + GELU hook, {form} kernel ({rem})"
    if form == "whole":      # fp32 taps, the 1.5e-7 erf: exact, rounded once
        c.round(what, got, exact)
    else:
        model = F.bf16(F.dw_gelu_model(x64, w64, b64, G, False)).reshape(batch * N, ch)
        c.modelled(what, got, exact, model, batch, pixels=True)
    _check_guard(c, guard)
    out2, _ = run()
    c.equal("second run (bitwise)", out2.view(torch.int16).double(), out.view(torch.int16).double())
    _recorded(lambda: FS.report(c))


# ---- b. the attention hook alone ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,family", [(n, f) for n in HG.ATTN_NS for f in HG.attn_families(n)])
def test_attention_hook(N, family):
    from transformer_latent_diffusion_amd import _lib
    dev = _dev()
    B, H = HG.attn_bh(N)
    d = 64 * H
    q, k, v = (t.to(dev) for t in HG.attn_inputs(family, N))
    qk = torch.cat([q.reshape(B * N, d), k.reshape(B * N, d)], dim=1).bfloat16().contiguous()
    vt = v.view(B, N, d).permute(0, 2, 1).bfloat16().contiguous()                   # [B, H * 64, N]

    def run():
        buf, att, guard = _guarded(B * N, d, 32)
        _lib.check(_lib.lib().tld_debug_attention_fwd(qk.data_ptr(), vt.data_ptr(), buf.data_ptr(), B, N, H, 1, None,
                                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "tld_debug_attention_fwd")
        torch.cuda.synchronize()
        return att, guard
    att, guard = run()
    form, rem, single = HG.attention_class(N)
    c = GridChecks(f"att{N}", B, N, int(round(N ** 0.5)), H)
    exact, model = FS._attn_both(q.double(), k.double(), v.double(), H, False)
    c.modelled(f"attention hook, {family} ({form}, N % 128 = {rem}{', one chunk' if single else ''})", att.double(), exact.reshape(B * N, d),
               F.bf16(model).reshape(B * N, d), B, heads=True)
    _check_guard(c, guard)
    att2, _ = run()
    c.equal("second run (bitwise)", att2.view(torch.int16).double(), att.view(torch.int16).double())
    del exact, model
    _recorded(lambda: FS.report(c))


# ---- c. the engine ---------------------------------------------------------------------------------------------------------------------------------------
def _assert_paths(prefix, d, G, batch, **kw):
    """Every recorded run of a case (both engines of an fp8 case, every step of a sampler case) against the restated dispatch, bit by bit."""
    tags = [t for t in _PATHS if t == prefix or t.startswith(prefix + "/")]
    assert tags, prefix
    for t in tags:
        if kw.get("fp8"):
            kw["fp8_fused"] = t.endswith("/fused")
        HG.assert_paths(t, _PATHS[t], *HG.expected_paths(d, G, batch, _cus(), **kw))
        if G == 16 and HG.fused_up(G, 4 * d, kw.get("fp8", False)):      # one of the two 16 x 16 forms, by the launch's size
            assert _PATHS[t] >> HG.BIT_UP_16 & 1 or _PATHS[t] >> HG.BIT_UP_16_4W & 1, (t, hex(_PATHS[t]))


@pytest.mark.parametrize("fam,d,G,batch,fp8", HG.ENGINE, ids=[f"{f}-g{G}" for f, _, G, _, _ in HG.ENGINE])
def test_engine_stages(fam, d, G, batch, fp8):
    kw = FS._cfg(d, 2 * G, 2)
    tag = f"{fam}g{G}"
    gpw = HG.cross_row_form(d, G * G, batch, _cus())[1]
    if fp8:
        _recorded(lambda: F8.run_forward_case(tag, case=(kw, batch, batch, ("0", "1")), checks=_with_gpw(GridChecks8, gpw), paths=_PATHS))
    else:
        _recorded(lambda: FS.run_forward_case(tag, case=(kw, (batch,), batch, {}, 0), checks=_with_gpw(GridChecks, gpw), paths=_PATHS))
    _assert_paths(tag, d, G, batch, fp8=fp8)


@pytest.mark.parametrize("G,batch", HG.PARTITION)
def test_cross_row_partition(G, batch):
    kw = FS._cfg(256, 2 * G, 1)
    tag = f"part{G}x{batch}"
    kind, gpw = HG.cross_row_form(256, G * G, batch, _cus())
    assert kind == "mfma"
    if _cus() == HG.CUS_MI355X:
        assert gpw == {(8, 128): 2, (24, 29): 4, (24, 15): 2}[(G, batch)]
    _recorded(lambda: FS.run_forward_case(tag, case=(kw, (batch,), batch, {}, 0), checks=_with_gpw(GridChecks, gpw), paths=_PATHS))
    _assert_paths(tag, 256, G, batch)


@pytest.mark.parametrize("G", HG.SAMPLER_GRIDS)
def test_sampler_grids(G):
    B = HG.SAMPLER_B
    kw = FS._cfg(256, 2 * G, 2)
    tag = f"s{G}"
    gpw = HG.cross_row_form(256, G * G, 2 * B, _cus())[1]
    _recorded(lambda: FS._sampler(tag, True, False, case=(kw, B, 3, (0, 1, 2)), checks=_with_gpw(GridChecks, gpw), paths=_PATHS))
    steps = [t for t in _PATHS if t.startswith(f"{tag}/dpm/step")]
    assert len(steps) == 3, steps
    _assert_paths(f"{tag}/dpm", 256, G, 2 * B, sampler=True)
    gc.collect()

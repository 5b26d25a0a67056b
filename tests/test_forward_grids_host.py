"""Host: the grid-dependent dispatch of the inference forward restated in Python, the case tables of tests/test_gpu_forward_grids.py held against it,
the pixel / query-row class masks of that file, and the input families whose bite is a property of the inputs alone.

tld_engine_create accepts any square token grid whose side G is a multiple of 4; what a forward launches at a grid follows from a handful of rules:

| dispatch                          | depends on              | restated as          | source                                         |
| attention form, N % 128           | token count             | attention_class      | plan_attention (tld_launch_plan.h)             |
| depthwise form, G % 16 / G % 3 /  | G                       | depthwise_class      | plan_dwconv (tld_launch_plan.h)                |
|   strip count                     |                         |                      |                                                |
| cross_row form and gpw            | d, ntok, batch, CUs     | cross_row_form       | plan_cross_row (tld_launch_plan.h)             |
| embed, LayerNorm-1, tail forms    | d, patch, operand type  | expected_paths       | plan_embed, plan_layernorm, plan_tail          |
| fused up-projection               | G, hid (bf16 only)      | fused_up             | plan (tld_body_plan.h)                         |
| fused QKV + attention             | ntok, d, LayerNorm-1    | fused_qkv_attention  | plan (tld_body_plan.h)                         |
|                                   | fold                    |                      |                                                |

The first three are restated in tests/launch_plan_ref.py, which tests/test_launch_plan_host.py holds against the compiled header field by field.
expected_paths turns them into the bits of tld_engine_debug_paths a forward must and must not set; the GPU file asserts them case by case, so a grid
that silently takes another kernel fails there.  The tests here hold: the two plan rules against tests/body_plan_ref.py; that the case tables reach
every value of every class (whole-image depthwise with G % 3 = 0, 1, 2; tiled with G % 16 = 0, 4, 8, 12; streaming with 1, 2, 3 strips; attention at
64 and 256 tokens, chunked, masked with N % 128 = 16 and 64 and with a single partial chunk; gpw 1, 2, 4 at a group count that is no power of two, on
the 256 CUs of an MI355X); that every class mask is non-empty where its class applies and absent where it does not; that removing the peaked key of
the two tail-peaked attention families moves the float64 output by more than ten times the rounding model's own error; and the depthwise hook's
refusal of a side that is no multiple of 4, in the engine's words, before any HIP call.
"""
import ctypes as C

import pytest
import torch

import body_plan_ref as BP
import infer_stage_refs as F
import train_stage_refs as R
from launch_plan_ref import attention_class, cross_row_form, depthwise_class

CUS_MI355X = 256

# ---- bits of tld_engine_debug_paths (Denoiser.PATH_NAMES / FP8_PATH_NAMES) ---------------------------------------------------------------------
BIT_QKV_ATTN, BIT_ATT_256, BIT_ATT_CHUNKED, BIT_ATT_64, BIT_ATT_MASKED = 11, 14, 15, 17, 19
BIT_CROSS_MFMA1, BIT_GPW1, BIT_GPWN, BIT_CROSS_VALU, BIT_FANOUT = 20, 24, 25, 26, 27
BIT_UP_16, BIT_UP_32, BIT_UP_16_4W, BIT_UP_ALONE, BIT_DW_WHOLE, BIT_DW_TILED, BIT_DW_STREAM = 28, 29, 30, 31, 32, 33, 34
BIT_F8_PASS, BIT_F8_CROSS, BIT_F8_DW_TILED, BIT_F8_DW_STREAM = 54, 55, 56, 57
BIT_EMBED_PLAIN, BIT_EMBED_MFMA1, BIT_LN_Q4_1, BIT_LN_GENERIC, BIT_LN_MX8, BIT_TAIL_FOLD, BIT_TAIL_MFMA1, BIT_TAIL_PLAIN = 0, 1, 5, 9, 10, 16, 45, 49
BIT_SPLITK_FINISH12, BIT_SPLITK_FINISH6 = 43, 44
EMBED_BITS = {BIT_EMBED_PLAIN} | {BIT_EMBED_MFMA1 + k for k in range(4)}
LN_BITS = {BIT_LN_GENERIC, BIT_LN_MX8} | {BIT_LN_Q4_1 + k for k in range(4)}
TAIL_BITS = {BIT_TAIL_PLAIN, BIT_TAIL_FOLD} | {BIT_TAIL_MFMA1 + k for k in range(4)}
ATT_BITS = {"256": BIT_ATT_256, "chunked": BIT_ATT_CHUNKED, "64": BIT_ATT_64, "masked": BIT_ATT_MASKED}
DW_BITS = {"whole": BIT_DW_WHOLE, "tiled": BIT_DW_TILED, "streaming": BIT_DW_STREAM}


# ---- the dispatch, restated: the three launch classes are in tests/launch_plan_ref.py, held against csrc/tld_launch_plan.h by tests/test_launch_plan_host.py ----
def fold_ln1(d, fp8=False):
    return not fp8 and d % 192 == 0 and d // 96 <= 8 and (3 * d) % 256 == 0


def fused_up(G, hid, fp8=False):
    """The depthwise conv + GELU in the up-projection's epilogue: the stand-alone depthwise kernels do not run."""
    return not fp8 and G in (16, 32) and hid % 256 == 0


def fused_qkv_attention(ntok, d, fp8=False):
    return fold_ln1(d, fp8) and ntok == 256 and d % 128 == 0


def expected_paths(d, G, batch, cus, mult=4, fp8=False, fp8_fused=True, sampler=False, pd=16):
    """(bits a forward of `batch` samples must set, bits it must not set).  batch: the samples cross_row sees (both halves of a CFG step).  pd: the patch's
    elements (every case here: 4 channels, 2 x 2 pixels)."""
    n, hid = G * G, d * mult
    on, off = set(), set()
    form = attention_class(n)[0]
    if fused_qkv_attention(n, d, fp8):
        on.add(BIT_QKV_ATTN); off |= set(ATT_BITS.values())
    else:
        on.add(ATT_BITS[form]); off |= {b for f, b in ATT_BITS.items() if f != form} | {BIT_QKV_ATTN}
    dw = depthwise_class(G)[0]
    if fused_up(G, hid, fp8):
        off |= set(DW_BITS.values()) | {BIT_UP_ALONE} | ({BIT_UP_32} if G == 16 else {BIT_UP_16, BIT_UP_16_4W})
        if G == 32:
            on.add(BIT_UP_32)
    else:
        on |= {DW_BITS[dw], BIT_UP_ALONE}; off |= {b for f, b in DW_BITS.items() if f != dw} | {BIT_UP_16, BIT_UP_32, BIT_UP_16_4W}
    kind, gpw = cross_row_form(d, n, batch, cus)
    if kind == "mfma":
        on |= {BIT_CROSS_MFMA1 + d // 256 - 1, BIT_GPW1 if gpw == 1 else BIT_GPWN}
        off |= {BIT_CROSS_VALU, BIT_GPWN if gpw == 1 else BIT_GPW1} | ({BIT_CROSS_MFMA1 + k for k in range(4)} - {BIT_CROSS_MFMA1 + d // 256 - 1})
    else:
        on.add(BIT_CROSS_VALU); off |= {BIT_CROSS_MFMA1 + k for k in range(4)} | {BIT_GPW1, BIT_GPWN}
    (on if sampler else off).add(BIT_FANOUT)
    f8 = {BIT_F8_DW_TILED: fp8 and fp8_fused and dw == "tiled", BIT_F8_DW_STREAM: fp8 and fp8_fused and dw == "streaming",
          BIT_F8_CROSS: fp8 and fp8_fused and d in (256, 512, 768),
          BIT_F8_PASS: fp8 and (not fp8_fused or dw == "whole" or d not in (256, 512, 768))}
    for b, v in f8.items():
        (on if v else off).add(b)
    # embed: the matrix-pipe kernel at a 16-element patch and d = 256 k (the engine always holds its split-bf16 weight), else the plain one
    embed = BIT_EMBED_MFMA1 + d // 256 - 1 if pd == 16 and d % 256 == 0 and d <= 1024 else BIT_EMBED_PLAIN
    on.add(embed); off |= EMBED_BITS - {embed}
    # LayerNorm-1: no kernel of its own where it is folded into the QKV GEMM; the quantising one in the fused fp8 mode at 256, 512, 768; four features per lane at 256 k
    if fold_ln1(d, fp8):
        off |= LN_BITS
    else:
        ln = BIT_LN_MX8 if fp8 and fp8_fused and d in (256, 512, 768) else BIT_LN_Q4_1 + d // 256 - 1 if d in (256, 512, 768, 1024) else BIT_LN_GENERIC
        on.add(ln); off |= LN_BITS - {ln}
    # the tail: bf16 operands fold the last down projection into it (any width); fp8 takes the matrix-pipe kernel where its weight image fits, else the plain one
    nt = BIT_TAIL_MFMA1 + (pd + 15) // 16 - 1
    tail = {nt, BIT_TAIL_FOLD} if not fp8 else {nt} if d % 128 == 0 and pd * d <= 40960 else {BIT_TAIL_PLAIN}
    on |= tail; off |= TAIL_BITS - tail
    off |= {BIT_SPLITK_FINISH12, BIT_SPLITK_FINISH6}                  # (no case here runs a low-latency class)
    return on, off


def assert_paths(tag, mask, on, off):
    bad = [f"bit {b} not set" for b in sorted(on) if not mask >> b & 1] + [f"bit {b} set" for b in sorted(off) if mask >> b & 1]
    assert not bad, f"{tag}: launch paths {mask:#x}: " + ", ".join(bad)


# ---- the case tables of tests/test_gpu_forward_grids.py ---------------------------------------------------------------------------------------------
GRIDS = list(range(4, 65, 4))                                         # every engine grid up to 64 x 64 tokens


def batch_of(G):
    return 3 if G <= 40 else 2                                        # 3 G^2 is no multiple of 256 at most grids: a partial last 256-row tile


DW_HOOK = [(G, batch_of(G), ch) for G in GRIDS + [96] for ch in (64, 128)]            # 96: three strips, the middle one with a halo on both sides
ATTN_NS = [16 * k * k for k in range(1, 17)]                          # every engine token count up to 4096


def attn_bh(n):
    return (3, 2) if n <= 1600 else (1, 2)


ATTN_FAMILIES = ("random", "rising", "negative", "positive", "peak last", "peak chunk")


def attn_families(n):
    """The families run at n tokens: the second tail-peaked family needs a partial last chunk (its key is N - N % 128)."""
    return [f for f in ATTN_FAMILIES if f != "peak chunk" or attention_class(n)[0] == "masked"]


ENGINE = ([("d256", 256, G, batch_of(G), False) for G in GRIDS] + [("d192", 192, G, batch_of(G), False) for G in GRIDS]
          + [("fp8", 256, G, batch_of(G), True) for G in (4, 12, 20, 28, 36, 44)])
# cross_row's partition at d = 256, one block, (G, batch): on 256 CUs gpw 2 with four groups per sample; gpw 4 with 36 groups (nine workgroups per
# sample); gpw 2 with 36 groups (the sweep has gpw 2 only at 64 x 64 tokens, 256 groups)
PARTITION = [(8, 128), (24, 29), (24, 15)]
SAMPLER_GRIDS = (12, 20, 28)                                          # DPM-Solver++, three steps, CFG with layer-0 sharing, d = 256
SAMPLER_B = 3


# ---- class masks ------------------------------------------------------------------------------------------------------------------------------------------
def pixel_classes(G):
    """{class: bool [G, G]} of the depthwise kernel the grid takes; only the classes that apply."""
    yy, xx = torch.meshgrid(torch.arange(G), torch.arange(G), indexing="ij")
    ey, ex = (yy == 0) | (yy == G - 1), (xx == 0) | (xx == G - 1)
    m = {"corner": ey & ex, "edge": ey ^ ex}
    if G > 2:
        m["interior"] = ~(ey | ex)
    form, rem = depthwise_class(G)
    if form == "tiled":
        m["16 x 16 tile seam"] = (yy % 16 == 15) | (yy % 16 == 0) | (xx % 16 == 15) | (xx % 16 == 0)
        if rem:
            m["partial tiles"] = F.dw_partial_tile_mask(G)
            m["partial tiles, outermost column"] = xx == G - 1
            m["partial tiles, lowest row"] = yy == G - 1
    elif form == "streaming":
        m["strip seam columns"] = (xx % 32 == 0) | (xx % 32 == 31)
    elif rem:
        m[f"last {rem} column(s) of the rotation"] = xx >= G - rem
    return m


def query_classes(n):
    """{class: bool [n]} over the query rows of one sample: first and last row, and for the masked kernel the last partial 128-query block and
    its first 32-row wave."""
    t = torch.arange(n)
    m = {"first query": t == 0, "last query": t == n - 1}
    form, rem, _ = attention_class(n)
    if form == "masked":
        m["partial query block"] = t >= n - rem
        m["partial query block, first wave"] = (t >= n - rem) & (t < n - rem + 32)
    return m


# ---- attention inputs -----------------------------------------------------------------------------------------------------------------------------------
PEAK = 1.5               # the peaked key's offset along the queries' common direction: its score leads the others by 8 PEAK = 12 nats


def attn_inputs(family, n):
    """(q, k, v) fp32 host tensors [B, n, 64 H], bf16-exact.  random / rising / negative / positive are families 1, 4, 5 and 5 mirrored of
    test_gpu_attn_bwd_classes.inputs; the tail-peaked families have every query along one direction and one key far along it: key n - 1, the
    last valid one, or key n - n % 128, the first of the partial chunk."""
    from test_gpu_attn_bwd_classes import _bf, inputs
    bh = attn_bh(n)
    if family in ("random", "rising", "negative", "positive"):
        fam, var = {"random": (1, 0), "rising": (4, 0), "negative": (5, 0), "positive": (5, 1)}[family]
        return inputs(fam, n, var, bh=bh)[:3]
    B, H = bh
    gen = torch.Generator().manual_seed(7000 + n + (1 if family == "peak chunk" else 0))
    rn = lambda *s: torch.randn(*s, generator=gen)
    q, k, v = 1.0 + 0.25 * rn(B, n, 64 * H), 0.25 * rn(B, n, 64 * H), rn(B, n, 64 * H)
    k[:, peaked_key(family, n)] += PEAK
    return _bf(q), _bf(k), _bf(v)


def peaked_key(family, n):
    return n - 1 if family == "peak last" else n - n % 128


# ---- tests ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_plan_rules_match_the_body_plan():
    from types import SimpleNamespace as NS
    for d in (192, 256, 384, 512, 768):
        for G in GRIDS:
            for fp8 in (False, True):
                if fp8 and d % 128:
                    continue
                sh = NS(d=d, L=2, H=d // 64, grid=G, ntok=G * G, hid=4 * d)
                sw = BP.switches({"TLD_FOLD_LN1": "0", "TLD_FOLD_LN3": "0", "TLD_FUSE_DWCONV": "0"} if fp8 else None)
                p = BP.plan(sh, sw, fp8, 0, 3, CUS_MI355X)
                assert p.fuse_dw == fused_up(G, 4 * d, fp8) and p.fused_qa == fused_qkv_attention(G * G, d, fp8) and p.fold_ln1 == fold_ln1(d, fp8), (d, G, fp8)
                assert p.dw_mx8 == (fp8 and G > 16)


def test_case_tables_reach_every_class():
    assert GRIDS == [4 * k for k in range(1, 17)] and ATTN_NS == [G * G for G in GRIDS]
    dw = {depthwise_class(G) for G, _, _ in DW_HOOK}
    assert dw == {("whole", 0), ("whole", 1), ("whole", 2), ("tiled", 0), ("tiled", 4), ("tiled", 8), ("tiled", 12),
                  ("streaming", 1), ("streaming", 2), ("streaming", 3)}, dw
    assert {ch for _, _, ch in DW_HOOK} == {64, 128} and all(b == (3 if G <= 40 else 2) for G, b, _ in DW_HOOK)
    for fam, fp8 in (("d256", False), ("d192", False)):           # the engine: the fused up-projection takes 16 and 32 away from the stand-alone kernels
        got = {depthwise_class(G) for f, d, G, _, _ in ENGINE if f == fam and not fused_up(G, 4 * d)}
        assert got == dw - {("streaming", 1), ("streaming", 3)}, (fam, got)
    assert {depthwise_class(G) for f, _, G, _, _ in ENGINE if f == "fp8"} == {("whole", 1), ("whole", 0), ("tiled", 4), ("tiled", 12)}
    att = {attention_class(n) for n in ATTN_NS}
    assert att == {("64", 0, False), ("256", 0, False), ("chunked", 0, False), ("masked", 16, True), ("masked", 16, False), ("masked", 64, False)}, att
    assert {attention_class(G * G) for fam, _, G, _, _ in ENGINE if fam != "fp8"} == att
    assert all(attn_bh(n) == ((3, 2) if n <= 1600 else (1, 2)) for n in ATTN_NS)
    for n in ATTN_NS:
        assert ("peak chunk" in attn_families(n)) == (attention_class(n)[0] == "masked") and len(attn_families(n)) >= 5
    # cross_row on 256 CUs: both forms; gpw 1, 2 and 4 at a group count that is no power of two
    forms = {(G * G // 16, cross_row_form(d, G * G, b, CUS_MI355X)) for _, d, G, b, _ in ENGINE} | {(G * G // 16, cross_row_form(256, G * G, b, CUS_MI355X)) for G, b in PARTITION}
    odd = {gpw for gps, (kind, gpw) in forms if kind == "mfma" and gps & (gps - 1)}
    assert odd == {1, 2, 4}, forms
    assert {kind for _, (kind, _) in forms} == {"mfma", "valu"}
    assert [cross_row_form(256, G * G, b, CUS_MI355X) for G, b in PARTITION] == [("mfma", 2), ("mfma", 4), ("mfma", 2)]
    assert [G * G // 16 // cross_row_form(256, G * G, b, CUS_MI355X)[1] for G, b in PARTITION] == [2, 9, 18]        # workgroups per sample
    # a partial last 256-row tile at most cases
    part = [G for _, _, G, b, _ in ENGINE if (b * G * G) % 256]
    assert len(part) > len(ENGINE) // 2
    assert all(depthwise_class(G)[0] != "streaming" and attention_class(G * G)[0] == "masked" for G in SAMPLER_GRIDS)


def test_expected_paths_are_consistent():
    for fam, d, G, b, fp8 in ENGINE:
        for fused in ((True, False) if fp8 else (True,)):
            on, off = expected_paths(d, G, b, CUS_MI355X, fp8=fp8, fp8_fused=fused)
            assert not on & off, (fam, G, on & off)
            assert len(on & set(ATT_BITS.values())) == 1 and len(on & set(DW_BITS.values())) == (0 if fused_up(G, 4 * d, fp8) else 1)
    on, off = expected_paths(256, 12, 2 * SAMPLER_B, CUS_MI355X, sampler=True)
    assert BIT_FANOUT in on and {BIT_ATT_MASKED, BIT_DW_WHOLE, BIT_CROSS_MFMA1, BIT_GPW1, BIT_UP_ALONE} <= on
    on, off = expected_paths(256, 32, 3, CUS_MI355X)
    assert BIT_UP_32 in on and {BIT_DW_STREAM, BIT_UP_ALONE} <= off and BIT_ATT_CHUNKED in on
    on, off = expected_paths(768, 16, 128, CUS_MI355X)                # the bench shape: fused QKV + attention, gpw 8
    assert {BIT_QKV_ATTN, BIT_CROSS_MFMA1 + 2, BIT_GPWN} <= on and BIT_ATT_256 in off and cross_row_form(768, 256, 128, CUS_MI355X) == ("mfma", 8)
    on, off = expected_paths(256, 20, 3, CUS_MI355X, fp8=True)
    assert {BIT_F8_DW_TILED, BIT_DW_TILED} <= on and {BIT_F8_PASS, BIT_F8_DW_STREAM} <= off
    on, off = expected_paths(256, 12, 3, CUS_MI355X, fp8=True)
    assert {BIT_F8_PASS, BIT_DW_WHOLE} <= on and BIT_F8_DW_TILED in off


@pytest.mark.parametrize("G", GRIDS + [96])
def test_pixel_class_masks(G):
    m = pixel_classes(G)
    form, rem = depthwise_class(G)
    assert all(v.shape == (G, G) and v.dtype == torch.bool and bool(v.any()) for v in m.values()), {k: int(v.sum()) for k, v in m.items()}
    assert int(m["corner"].sum()) == 4 and int(m["edge"].sum()) == 4 * (G - 2) and int(m["interior"].sum()) == (G - 2) ** 2
    assert bool((m["corner"] ^ m["edge"] ^ m["interior"]).all())
    tags = set(m) - {"corner", "edge", "interior"}
    if form == "whole":
        assert tags == ({f"last {rem} column(s) of the rotation"} if rem else set())
        if rem:
            assert int(m[f"last {rem} column(s) of the rotation"].sum()) == rem * G
    elif form == "streaming":
        assert tags == {"strip seam columns"} and int(m["strip seam columns"].sum()) == 2 * rem * G
    else:
        assert tags == {"16 x 16 tile seam"} | ({"partial tiles", "partial tiles, outermost column", "partial tiles, lowest row"} if rem else set())
        if rem:
            cut = G - G % 16
            want = torch.tensor([[x >= cut or y >= cut for x in range(G)] for y in range(G)])
            assert torch.equal(m["partial tiles"], want) and int(want.sum()) == G * G - cut * cut
            assert bool((m["partial tiles, outermost column"] <= m["partial tiles"]).all()) and int(m["partial tiles, outermost column"].sum()) == G
            assert bool((m["partial tiles, lowest row"] <= m["partial tiles"]).all()) and int(m["partial tiles, lowest row"].sum()) == G
    assert (F.dw_partial_tile_mask(G) is None) == (G % 16 == 0)


@pytest.mark.parametrize("n", ATTN_NS)
def test_query_class_masks(n):
    m = query_classes(n)
    form, rem, single = attention_class(n)
    assert all(v.shape == (n,) and bool(v.any()) for v in m.values())
    assert int(m["first query"].sum()) == 1 and int(m["last query"].sum()) == 1
    if form == "masked":
        assert rem in (16, 64) and int(m["partial query block"].sum()) == rem and int(m["partial query block, first wave"].sum()) == min(rem, 32)
        assert bool(m["partial query block"][-1]) and not bool(m["partial query block"][:n - rem].any())
        assert single == (n == 16)
    else:
        assert set(m) == {"first query", "last query"} and n % 128 in (0, 64)


@pytest.mark.parametrize("n", [16, 144, 400, 576])
@pytest.mark.parametrize("family", ["peak last", "peak chunk"])
def test_tail_peaked_families_bite(family, n):
    """Removing the peaked key moves the float64 output, over the whole tensor and in every query class, by more than ten times the rounding
    model's error there; the key holds most of every query's weight."""
    B, H = attn_bh(n)
    q, k, v = (t.double() for t in attn_inputs(family, n))
    exact = R.attn_fwd(q, k, v, H)
    model = F.bf16(F.attn_model(q, k, v, H))
    key = peaked_key(family, n)
    assert 0 <= key < n and (family == "peak last" or key % 128 == 0)
    keep = torch.ones(n, dtype=torch.bool)
    keep[key] = False
    without = R.attn_fwd(q, k[:, keep], v[:, keep], H)
    s = R._heads(q, H) @ R._heads(k, H).transpose(-1, -2) / 8.0
    p = torch.softmax(s, -1)[..., key]
    assert 0.5 < float(p.min()), float(p.min())
    rel = lambda a, rows: float((a - exact)[:, rows].norm() / exact[:, rows].norm())
    for tag, rows in {"whole": torch.ones(n, dtype=torch.bool), **query_classes(n)}.items():
        yard, moved = rel(model, rows), rel(without, rows)
        assert moved > 10 * yard and yard > 0, (tag, moved, yard)


def test_depthwise_hook_refuses_a_side_that_is_no_multiple_of_4_in_the_engine_s_words():
    """Before any HIP call: pointers that are never dereferenced.  Sides 20 and 28 pass the grid rule and reach the size rule behind it."""
    from transformer_latent_diffusion_amd import _lib
    L = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)
    fp = C.cast(p, C.POINTER(C.c_float))
    for G in (18, 6, 17, 30, 50):
        assert L.tld_debug_dwconv_gelu(p, fp, fp, p, 1, G, 64, None) == 1, G
        err = L.tld_last_error()
        assert f"token count {G * G} unsupported: image_size / patch_size must be a multiple of 4".encode() in err, err
        cfg = BP.NS(embed_dim=64, patch_size=1, image_size=G, n_channels=4, noise_embed_dims=256, n_layers=1, mlp_multiplier=4, text_emb_size=768)
        assert BP.config_check(cfg, 1).encode() in err                # the engine's own refusal of that grid
    for G in (20, 28):
        assert L.tld_debug_dwconv_gelu(p, fp, fp, p, 12000000, G, 3072, None) == 1
        assert b"workgroups" in L.tld_last_error() and f"grid {G}".encode() in L.tld_last_error(), L.tld_last_error()

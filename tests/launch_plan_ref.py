"""The launches of the inference forward's row and attention kernels, restated in Python: what csrc/tld_launch_plan.h decides
per launch site -- form, template instantiation, partition, grid, block, dynamic LDS bytes, launch-path bits -- held against the header field by field
(tests/test_launch_plan_host.py); and the three class functions the grid tests read (tests/test_forward_grids_host.py).  No numpy, no GPU.

Every plan_* returns a dict whose keys are FIELDS[site], in the order tests/host/launch_plan_main.cpp prints them.
"""
LDS_LIMIT = 160 * 1024
GRID_YZ, GRID_X = 65535, 2 ** 31 - 1

# bits of tld_engine_debug_paths (the EP_* enum)
EP_EMBED_PLAIN, EP_EMBED_MFMA, EP_LN_Q4, EP_LN_GENERIC, EP_LN_MX8 = 0, 1, 5, 9, 10
EP_ATT_256, EP_ATT_CHUNKED, EP_TAIL_FOLD, EP_ATT_64, EP_ATT_MASKED = 14, 15, 16, 17, 19
EP_CROSS_MFMA, EP_CROSS_GPW1, EP_CROSS_GPWN, EP_CROSS_VALU, EP_CROSS_FANOUT = 20, 24, 25, 26, 27
EP_DW_WHOLE, EP_DW_TILED, EP_DW_STREAM, EP_SPLITK_FINISH12, EP_SPLITK_FINISH6, EP_TAIL_MFMA, EP_TAIL_PLAIN = 32, 33, 34, 43, 44, 45, 49
EP_CROSS_F8, EP_DW_TILED_F8, EP_DW_STREAM_F8 = 55, 56, 57
# every bit some plan of the header can set
OWNED = ({EP_EMBED_PLAIN, EP_LN_GENERIC, EP_LN_MX8, EP_ATT_256, EP_ATT_CHUNKED, EP_TAIL_FOLD, EP_ATT_64, EP_ATT_MASKED, EP_CROSS_GPW1, EP_CROSS_GPWN, EP_CROSS_VALU,
          EP_CROSS_FANOUT, EP_DW_WHOLE, EP_DW_TILED, EP_DW_STREAM, EP_SPLITK_FINISH12, EP_SPLITK_FINISH6, EP_TAIL_PLAIN, EP_CROSS_F8, EP_DW_TILED_F8, EP_DW_STREAM_F8}
         | {b + k for b in (EP_EMBED_MFMA, EP_LN_Q4, EP_CROSS_MFMA, EP_TAIL_MFMA) for k in range(4)})

GEOM = ("form", "gx", "gy", "gz", "block", "groups", "lds", "paths")
FIELDS = {"embed": GEOM + ("tpw", "nj", "half"), "ln": GEOM + ("nq", "nj", "half"), "cross": GEOM + ("nq", "gpw", "nj", "cps", "half", "mode_outputs"),
          "skf": GEOM + ("cpl",), "tail": GEOM + ("nt", "rt", "nj", "rows_per_block", "half"), "dw": GEOM + ("f8",), "attn": GEOM + ("kt", "nw", "nbuf", "npairs")}
EMBED_FORMS, LN_FORMS, CROSS_FORMS, SKF_FORMS = ("plain", "mfma"), ("none", "q4", "generic", "mx8"), ("valu", "mfma"), ("none", "cpl12", "cpl6")
TAIL_FORMS, DW_FORMS, ATT_FORMS = ("plain", "mfma", "fold"), ("whole", "tiled", "streaming"), ("256", "chunked", "one chunk", "masked")


def _bits(*bits):
    return sum(1 << b for b in bits)


def _plan(site, form, groups, block, lds, paths, grid=None, **kw):
    """A plan of one launch site; a launch over rows has its workgroups on x alone (the extent is the count's low 32 bits)."""
    gx, gy, gz = grid if grid else (groups & 0xFFFFFFFF, 1, 1)
    p = dict.fromkeys(FIELDS[site], 0)
    p.update(form=form, gx=gx, gy=gy, gz=gz, block=block, groups=groups, lds=lds, paths=paths, **{k: int(v) for k, v in kw.items()})
    assert set(p) == set(FIELDS[site])
    return p


def _ceil(a, b):
    return -(-a // b)


def plan_embed(batch, ntok, pd, cpp, d, held):
    """32 token rows per workgroup.  The matrix-pipe kernel: the split-bf16 Linear weight held, a 16-element patch, d a multiple of 256."""
    groups = _ceil(batch * ntok, 32)
    if held and pd == 16 and cpp == 16 and d % 256 == 0 and d <= 1024:
        return _plan("embed", 1, groups, 256, 1024 + 2048 + 12 * d + 18432, _bits(EP_EMBED_MFMA + d // 256 - 1), tpw=d // 128)
    return _plan("embed", 0, groups, 256, 4 * pd * (d + cpp), _bits(EP_EMBED_PLAIN), nj=_ceil(d, 128), half=d % 128 != 0)


def plan_layernorm(M, d, mx8):
    """Four rows per workgroup.  Four features per lane at d = 256 k; the quantising kernel at 256, 512, 768 and nowhere else ("none")."""
    groups = _ceil(M, 4)
    if mx8:
        ok = d in (256, 512, 768)
        return _plan("ln", 3 if ok else 0, groups, 256, 0, _bits(EP_LN_MX8), nq=d // 256 if ok else 0)
    if d in (256, 512, 768, 1024):
        return _plan("ln", 1, groups, 256, 0, _bits(EP_LN_Q4 + d // 256 - 1), nq=d // 256)
    return _plan("ln", 2, groups, 256, 0, _bits(EP_LN_GENERIC), nj=_ceil(d, 128), half=d % 128 != 0)


def plan_cross_row(batch, ntok, d, heads, x_in, f8, cus):
    """Matrix-pipe form (d = 256 k): gpw groups of 16 rows per workgroup -- the largest power of two (<= 16) that divides a sample's groups and leaves a
    workgroup per CU.  Else the VALU form: cps chunks per sample, one resident round of three workgroups per CU where the batch allows."""
    fan = [EP_CROSS_FANOUT] if x_in else []
    if d % 256 == 0 and d <= 1024 and ntok % 16 == 0:
        gps, gpw = ntok // 16, 1
        while gpw < 16 and gps % (gpw * 2) == 0 and batch * (gps // (gpw * 2)) >= cus:
            gpw *= 2
        paths = _bits(EP_CROSS_MFMA + d // 256 - 1, EP_CROSS_GPW1 if gpw == 1 else EP_CROSS_GPWN, *fan, *([EP_CROSS_F8] if f8 else []))
        return _plan("cross", 1, batch * (gps // gpw), 512, 64 * d + 8192 + 8 * d, paths, nq=d // 256, gpw=gpw, mode_outputs=d in (256, 512, 768))
    slots, rows = 3 * cus, batch * ntok
    k = _ceil(rows, slots * 48)
    cps = max(1, min(slots * k // batch, max(ntok // 8, 1)))
    return _plan("cross", 0, batch * cps, 256, 4 * (heads * d + 2 * d + heads), _bits(EP_CROSS_VALU, *fan), nj=_ceil(d, 128), half=d % 128 != 0, cps=cps)


def plan_splitk_finish(M, d):
    form = {768: 1, 384: 2}.get(d, 0)
    return _plan("skf", form, _ceil(M, 4), 256, 0, (0, _bits(EP_SPLITK_FINISH12), _bits(EP_SPLITK_FINISH6))[form], cpl=(0, 12, 6)[form])


def plan_tail(batch, ntok, pd, d, hid, held, cus):
    """Folded (the hidden activation given): rt 16-row tiles per workgroup, 4 (2 from three patch-feature tiles on) where every CU still gets a workgroup.
    Matrix-pipe: the split-bf16 weight held, d a multiple of 128, pd d <= 40960.  Else the plain kernel, 64 rows per workgroup."""
    rows, nt = batch * ntok, _ceil(pd, 16)
    if hid:
        big = 4 if nt <= 2 else 2
        rt = big if rows >= 16 * big * cus else 1
        return _plan("tail", 2, _ceil(rows, 16 * rt), 512, 8192 * rt * nt, _bits(EP_TAIL_MFMA + min(nt, 4) - 1, EP_TAIL_FOLD), nt=min(nt, 4), rt=rt)
    if held and d % 128 == 0 and pd * d <= 40960:
        return _plan("tail", 1, _ceil(rows, 64), 256, 64 * nt * d, _bits(EP_TAIL_MFMA + min(nt, 4) - 1), nt=min(nt, 4))
    return _plan("tail", 0, _ceil(rows, 64), 256, 4 * pd * d, _bits(EP_TAIL_PLAIN), nj=_ceil(d, 128), half=d % 128 != 0, rows_per_block=64)


def plan_dwconv(batch, grid, channels, f8):
    form, arg = depthwise_class(grid)
    chunks = channels // 64
    if form == "streaming":
        return _plan("dw", 2, batch * arg * chunks, 320, 0, _bits(EP_DW_STREAM, *([EP_DW_STREAM_F8] if f8 else [])), f8=f8)
    if form == "tiled":
        return _plan("dw", 1, batch * _ceil(grid, 16) ** 2 * chunks, 256, 0, _bits(EP_DW_TILED, *([EP_DW_TILED_F8] if f8 else [])), f8=f8)
    return _plan("dw", 0, batch * chunks, 256, grid * grid * 128, _bits(EP_DW_WHOLE))


def plan_attention(batch, ntok, heads):
    """One K chunk of kc keys and its V^T chunk take kc 128 + 64 (2 kc + 8) bytes; the 256-token kernel adds a transpose patch per wave."""
    stage = lambda kc: kc * 128 + 64 * (kc * 2 + 8)
    if ntok == 256:
        return _plan("attn", 0, heads * batch, 256, stage(256) + 4 * 16 * 144, _bits(EP_ATT_256), grid=(1, heads, batch), kt=8, nw=4, nbuf=1)
    if ntok % 256 == 0:
        pairs = batch * heads
        return _plan("attn", 1, _ceil(pairs, 8) * 8 * (ntok // 256), 256, 2 * 128 * 128 + 2 * 64 * 256 + 4 * 16 * 144, _bits(EP_ATT_CHUNKED), nbuf=1, npairs=pairs)
    if ntok in (128, 64, 32):          # the whole sample in one chunk; only 64 is a square grid's count and has a bit
        kt = ntok // 32
        return _plan("attn", 2, heads * batch, kt * 64, stage(ntok), _bits(EP_ATT_64) if ntok == 64 else 0, grid=(1, heads, batch), kt=kt, nw=kt, nbuf=1)
    qb, nbuf = _ceil(ntok, 128), 2 if ntok > 128 else 1
    return _plan("attn", 3, qb * heads * batch, 256, nbuf * stage(128), _bits(EP_ATT_MASKED), grid=(qb, heads, batch), kt=4, nw=4, nbuf=nbuf)


PLANS = {"embed": plan_embed, "ln": plan_layernorm, "cross": plan_cross_row, "skf": plan_splitk_finish, "tail": plan_tail, "dw": plan_dwconv, "attn": plan_attention}


# ---- the classes the grid tests read ------------------------------------------------------------------------------------------------------------------
def attention_class(n):
    """launch_attention: (form, N % 128, single partial chunk) -- the last two for the masked kernel (attn_kernel<4, 4, true>: 128-key chunks,
    128-query blocks, one K / V buffer when there is one chunk), else (form, 0, False).  128 and 32 tokens are no square grid's count."""
    if n == 256:
        return "256", 0, False
    if n % 256 == 0:
        return "chunked", 0, False
    if n == 64:
        return "64", 0, False
    assert n not in (128, 32) and n % 16 == 0, n
    return "masked", n % 128, n <= 128


def depthwise_class(G):
    """launch_dwconv_gelu: (form, what the form's loop ends on) -- whole image: G % 3 (the three-buffer column rotation); tiled: G % 16 (the width
    of the partial last tile, 0: none); streaming: the number of 32-column strips."""
    if G > 16 and G % 32 == 0:
        return "streaming", G // 32
    if G > 16:
        return "tiled", G % 16
    return "whole", G % 3


def cross_row_form(d, ntok, batch, cus):
    """launch_cross_row: ("mfma", gpw) -- groups of 16 rows per workgroup: the largest power of two (<= 16) that divides a sample's groups and
    leaves a workgroup per CU -- or ("valu", 1)."""
    p = plan_cross_row(batch, ntok, d, d // 64, False, False, cus)
    return (CROSS_FORMS[p["form"]], p["gpw"] if p["form"] else 1)

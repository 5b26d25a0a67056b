"""The mode of an inference engine, restated in Python: what csrc/tld_body_plan.h decides -- refusals, switches, the plan, the held
images, the reserved stages -- and, beside it, what run_body does WITH a plan: the images its launches read and the stages it snaps.  The first half is held
against the header field by field (tests/test_body_plan_host.py); the second half is what the header's tables are cross-checked with.  No numpy, no GPU.
"""
from types import SimpleNamespace as NS

ST_F32, ST_BF16, ST_U8, ST_MX8S = 0, 1, 2, 3
ST_BYTES = {ST_F32: 4, ST_BF16: 2, ST_U8: 1, ST_MX8S: 1}
RS = 2                                 # bytes of a residual-stream element (the bf16-residual build, the only one built)
LN_SLOTS = 8
LOWLAT_MAX_ROWS = {1: 4096, 2: 1024}
SWITCHES = ("TLD_FOLD_LN1", "TLD_FOLD_LN3", "TLD_FOLD_TAIL", "TLD_FUSE_DWCONV", "TLD_FUSE_QKV_ATTN", "TLD_FP8_FUSED")       # the six structural ones


def atoi(s):
    """C's atoi: leading white space, an optional sign, digits; anything else ends the number ("" and "on" are 0)."""
    s = s.lstrip(" \t\n\v\f\r")
    sign, k = 1, 0
    if s[:1] in ("+", "-"):
        sign, s = (-1 if s[0] == "-" else 1), s[1:]
    while k < len(s) and s[k] in "0123456789":
        k += 1
    return sign * int(s[:k]) if k else 0


def switches(env=None):
    env = env or {}
    on = lambda k: atoi(env[k]) != 0 if k in env else True
    return NS(fold_ln1=on("TLD_FOLD_LN1"), fold_ln3=on("TLD_FOLD_LN3"), fold_tail=on("TLD_FOLD_TAIL"), fuse_dwconv=on("TLD_FUSE_DWCONV"),
              fuse_qkv_attn=on("TLD_FUSE_QKV_ATTN"), fp8_fused=on("TLD_FP8_FUSED"), share_l0=on("TLD_SHARE_L0"), guidance_skip=on("TLD_GUIDANCE_SKIP"),
              qkv_pair=min(2, max(0, atoi(env["TLD_QKV_ATTN_PAIR"]))) if "TLD_QKV_ATTN_PAIR" in env else 1)


def shape(cfg):
    grid = cfg.image_size // cfg.patch_size
    return NS(d=cfg.embed_dim, L=cfg.n_layers, H=cfg.embed_dim // 64, grid=grid, ntok=grid * grid, pd=cfg.n_channels * cfg.patch_size ** 2,
              hid=cfg.mlp_multiplier * cfg.embed_dim, img=cfg.n_channels * cfg.image_size ** 2, ne=cfg.noise_embed_dims, text=cfg.text_emb_size)


def _cdiv(a, b):
    """C's integer division (towards zero) and remainder, for the refusals that see negative numbers."""
    q = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)
    return q, a - q * b


def config_check(cfg, max_batch, device_id=0, ndev=1):
    """tld_engine_create's refusals on the configuration, in order; "" when it is good."""
    d, p = cfg.embed_dim, cfg.patch_size
    if d <= 0 or _cdiv(d, 64)[1] != 0 or d > 1024:
        return (f"embed_dim={d} unsupported: must be a multiple of the head width 64 (n_heads = embed_dim // 64, tld/transformer_blocks.py:126-128) and <= 1024 "
                "(the row kernels hold a token row in 8 x 128-feature register groups)")
    if p <= 0 or _cdiv(cfg.image_size, p)[1] != 0:
        return f"image_size={cfg.image_size} must be divisible by patch_size={p}"
    grid = _cdiv(cfg.image_size, p)[0]
    ntok = grid * grid
    if ntok % 16 != 0:
        return f"token count {ntok} unsupported: image_size / patch_size must be a multiple of 4"
    pd = cfg.n_channels * p * p
    if pd > 64:
        return f"patch_dim={pd} > 64 unsupported"
    if _cdiv(cfg.noise_embed_dims, 2)[1] != 0 or cfg.noise_embed_dims <= 0:
        return "noise_embed_dims must be even"
    if max_batch <= 0 or cfg.n_layers <= 0 or cfg.mlp_multiplier <= 0 or cfg.text_emb_size <= 0:
        return "non-positive size in config"
    if (cfg.mlp_multiplier * d) % 64:
        return "hidden width must be a multiple of 64"
    hid_bytes = max_batch * ntok * cfg.mlp_multiplier * d * 2
    if hid_bytes >= 1 << 32:
        return f"max_batch={max_batch}: the hidden activation ({hid_bytes} bytes) must stay below 4 GiB; run larger batches as several calls"
    # what the hidden-activation rule alone does not hold (csrc/tld_reach.h: body_reach_check)
    qk_bytes = max_batch * ntok * 2 * d * 2
    if qk_bytes >= 1 << 32:
        return (f"max_batch={max_batch}: the q|k activation (max_batch x tokens x 2 embed_dim x 2 B = {qk_bytes} bytes) must stay below 4 GiB, the reach of the 32-bit "
                f"offsets it is addressed through; the largest max_batch that fits is {((1 << 32) - 1) // (ntok * 2 * d * 2)}; run larger batches as several calls")
    if max_batch > 65535:
        return (f"max_batch={max_batch}: the self-attention kernels put one sample on each block of the grid's z axis (at most 65535); the largest max_batch that fits "
                "is 65535; run larger batches as several calls")
    if device_id < 0 or device_id >= ndev:
        return f"device_id {device_id} out of range ({ndev} devices)"
    H = d // 64
    lds = ((pd * d + pd * pd) * 4, pd * d * 4, (H * d + 2 * d + H) * 4)
    if max(lds) > 160 * 1024:
        return (f"embed_dim={d} with patch_dim={pd} needs {lds[0]} / {lds[1]} / {lds[2]} bytes of LDS in the embed / out-proj / cross-attention row kernels "
                f"(limit {160 * 1024} each): reduce patch_size*patch_size*n_channels or embed_dim")
    return ""


def class_refusal(sh, max_batch, cls, fp8):
    if cls == 0:
        return ""
    if cls not in (1, 2):
        return f"low-latency class {cls}: 0 = off, 1 = four K-splits (engines up to 4096 token rows), 2 = eight (up to 1024)"
    if fp8:
        return ("low-latency class: bf16 GEMM operands only -- this engine runs MX-fp8 GEMMs (tld_engine_set_gemm_dtype), whose down projection has no "
                "split-K form")
    rows = max_batch * sh.ntok
    if rows > LOWLAT_MAX_ROWS[cls]:
        why = "class 1 (four K-splits) is the faster one" if cls == 2 else "the default tiles fill the chip"
        return (f"low-latency class {cls}: engine capacity {rows} token rows (max_batch {max_batch} x {sh.ntok} tokens) exceeds {LOWLAT_MAX_ROWS[cls]} -- at that "
                f"size {why}")
    split = 4 * cls
    if sh.d not in (768, 384) or sh.hid % (64 * split):
        return f"low-latency class: needs embed_dim 384 or 768 (got {sh.d}) and a hidden width that splits into {split} multiples of 64 (got {sh.hid})"
    return ""


def dtype_refusal(sh, dtype, cls):
    if dtype not in (0, 1):
        return f"gemm dtype {dtype}: 0 = bf16, 1 = MX-fp8 (e4m3 + E8M0 block scales)"
    if dtype == 0:
        return ""
    if cls:
        return "fp8 GEMMs and the low-latency class exclude each other (the split-K down projection is bf16 only): clear tld_engine_set_low_latency first"
    if sh.d % 128 or sh.hid % 128:
        return "fp8 GEMMs need embed_dim and hidden width multiples of 128"
    return ""


def plan_qkv_pair(samples, heads, cus):
    """csrc/tld_qkv_pair_plan.h: two heads per tile where ceil(pairs / CUs) x 1.8 < ceil(items / CUs)."""
    if samples < 1 or heads < 2 or heads % 2 or cus < 1:
        return False
    items = samples * heads
    return -(-(items // 2) // cus) * 18 < -(-items // cus) * 10


def plan(sh, sw, fp8, cls, max_batch, cus, finalized=None):
    """Every structural decision, each rule once (the order follows the forward)."""
    p = NS(fp8=fp8, cls=cls, heads=sh.H, cus=cus, share_l0=sw.share_l0, guidance_skip=sw.guidance_skip)
    p.fold_ln1 = sw.fold_ln1 and not fp8 and sh.d % 192 == 0 and sh.d // 96 <= LN_SLOTS and (3 * sh.d) % 256 == 0
    p.fold_ln3 = sw.fold_ln3 and not fp8 and sh.hid % 256 == 0 and sh.d in (768, 512, 256)
    p.fused_qa = sw.fuse_qkv_attn and p.fold_ln1 and sh.ntok == 256 and sh.d % 128 == 0
    p.pair_always = sw.qkv_pair == 2
    if finalized is not None:
        p.pair_held = finalized.pair_held
    else:
        p.pair_held = (p.fused_qa and not cls and sh.H % 2 == 0 and sw.qkv_pair != 0
                       and (p.pair_always or any(plan_qkv_pair(b, sh.H, cus) for b in range(1, max_batch + 1))))
    p.pair = p.pair_held and p.fused_qa and not cls
    p.pair_slots = min(max_batch * (sh.H // 2), cus) if p.pair_held else 0
    p.fuse_dw = sw.fuse_dwconv and not fp8 and sh.grid in (16, 32) and sh.hid % 256 == 0
    p.seam = p.fuse_dw and sh.grid == 32
    p.fold_tail_held = sw.fold_tail and not fp8
    p.fold_tail = p.fold_tail_held and not cls
    fuse8 = fp8 and sw.fp8_fused
    p.ln_mx8, p.cross_mx8, p.dw_mx8 = fuse8 and sh.d in (256, 512, 768), fuse8 and sh.d in (768, 512, 256), fuse8 and sh.grid > 16
    p.quant_qkv, p.quant_up, p.quant_down = fp8 and not p.ln_mx8, fp8 and not p.cross_mx8, fp8 and not p.dw_mx8
    p.ll_split = 0 if fp8 else {0: 0, 1: 4, 2: 8}[cls]
    return p


def pair_launch(p, samples):
    return p.pair and (p.pair_always or plan_qkv_pair(samples, p.heads, p.cus))


def images(sh, p):
    """{member of Layer: (img.* stage name or "", element type, elements, margin, held)}"""
    d, hid = sh.d, sh.hid
    bf, f1, f3, qa, pr, f8 = not p.fp8, p.fold_ln1, p.fold_ln3, p.fused_qa, p.pair_held, p.fp8
    t = {"qkv_w": ("", ST_BF16, 3 * d * d, 0, bf and not f1), "up_w": ("", ST_BF16, hid * d, 0, bf and not f3), "down_w": ("", ST_BF16, d * hid, 0, bf),
         "kv_w": ("kv_w", ST_F32, 2 * d * d, 0, True), "q_w": ("q_w", ST_F32, d * d, 0, True), "up_b": ("up_b", ST_F32, hid, 0, True),
         "dw_b": ("dw_b", ST_F32, hid, 0, True), "down_b": ("down_b", ST_F32, d, 0, True)}
    for n in ("n1_w", "n1_b", "n2_w", "n2_b", "n3_w", "n3_b"):
        t[n] = (n, ST_F32, d, 0, True)
    t.update({"qkv_wf": ("qkv_wf", ST_BF16, 3 * d * d, 0, f1), "qkv_c1": ("qkv_c1", ST_F32, 3 * d, 0, f1), "qkv_b1": ("qkv_b1", ST_F32, 3 * d, 0, f1),
              "qkv_wp": ("qkv_wp", ST_BF16, 3 * d * d, 0, qa), "qkv_c1p": ("qkv_c1p", ST_F32, 3 * d, 64, qa), "qkv_b1p": ("qkv_b1p", ST_F32, 3 * d, 64, qa),
              "qkv_wp2": ("", ST_BF16, 3 * d * d, 0, pr), "qkv_c1p2": ("", ST_F32, 3 * d, 0, pr), "qkv_b1p2": ("", ST_F32, 3 * d, 0, pr),
              "up_wf": ("", ST_BF16, hid * d, 0, f3), "up_c1": ("", ST_F32, hid, 0, f3), "up_b1": ("", ST_F32, hid, 0, f3),
              "dw_w9c": ("dw_w9c", ST_F32, 9 * hid, 0, True), "dw_w9c_half": ("dw_w9c_half", ST_F32, 9 * hid, 0, True), "dw_b_half": ("dw_b_half", ST_F32, hid, 0, True),
              "dw_wpk": ("dw_wpk", ST_BF16, 24 * hid, 0, True),
              "qkv_w8": ("qkv_w8", ST_U8, 3 * d * d, 0, f8), "qkv_s8": ("qkv_s8", ST_MX8S, 3 * d * d // 32, 0, f8), "up_w8": ("up_w8", ST_U8, hid * d, 0, f8),
              "up_s8": ("up_s8", ST_MX8S, hid * d // 32, 0, f8), "down_w8": ("down_w8", ST_U8, d * hid, 0, f8), "down_s8": ("down_s8", ST_MX8S, d * hid // 32, 0, f8)})
    return t


# ---- what run_body does with a plan (csrc/tld_engine.hip): the second half of every cross-check -------------------------------------------------------------
def reads(sh, p, max_batch):
    """The members of Layer some launch of a forward reads (the debug row of the folded tail included)."""
    r = {"kv_w", "q_w", "n2_w", "n2_b", "n3_w", "n3_b", "down_b"}
    if not p.fold_ln1:
        r |= {"n1_w", "n1_b"}
    if p.fused_qa:
        r |= {"qkv_wp", "qkv_c1p", "qkv_b1p"}
        if any(pair_launch(p, b) for b in range(1, max_batch + 1)):
            r |= {"qkv_wp2", "qkv_c1p2", "qkv_b1p2"}
    elif p.fp8:
        r |= {"qkv_w8", "qkv_s8"}
    else:
        r |= {"qkv_wf", "qkv_c1", "qkv_b1"} if p.fold_ln1 else {"qkv_w"}
    if p.fp8:
        r |= {"up_w8", "up_s8", "up_b", "down_w8", "down_s8"}
    else:
        r |= {"up_wf", "up_c1", "up_b1"} if p.fold_ln3 else {"up_w", "up_b"}
        r |= {"down_w"}
    r |= {"dw_b_half", "dw_wpk"} if p.fuse_dw else {"dw_w9c", "dw_b", "dw_w9c_half", "dw_b_half"}
    return r


def snapped(sh, p, max_batch):
    """{stage: bytes} of every SNAP / sink of a forward of max_batch samples, and of the samplers' step.* stages."""
    B, M, d, hid = max_batch, max_batch * sh.ntok, sh.d, sh.hid
    s = {"tokens0": M * d * RS, "out": B * sh.img * 4}
    s.update({"step." + n: B * sh.img * 4 for n in ("x_t", "x0_prev", "x0", "x_next", "out")})
    for l in range(sh.L):
        b = {"x_in": M * d * RS, "att": M * d * 2, "sa": M * d * 4, "ca": M * d * RS}
        if p.fold_ln1:
            b["ln1"] = M * LN_SLOTS * 2 * 4
        elif not p.ln_mx8:
            b["xn1"] = M * d * 2
        if not p.fused_qa:
            b["qk"], b["vt"] = M * 2 * d * 2, M * d * 2
            if p.fp8:
                b["a8_qkv.q"], b["a8_qkv.s"] = M * d, M * d // 32
        if p.fold_ln3:
            b["stats"] = M * 2 * 4
        elif not p.cross_mx8:
            b["xn3"] = M * d * 2
        if not p.fuse_dw:
            b["hid_pre"] = M * hid * 2
            if p.fp8:
                b["a8_up.q"], b["a8_up.s"] = M * d, M * d // 32
        if not p.dw_mx8:
            b["hid"] = M * hid * 2
        if l + 1 == sh.L and p.fold_tail:
            b["mlp"] = M * d * 4                     # the fp32 debug row of the folded tail
        else:
            b["mlp"] = M * d * RS
            if p.ll_split:
                b["splitk"] = p.ll_split * M * d * 4
            elif p.fp8:
                b["a8_down.q"], b["a8_down.s"] = M * hid, M * hid // 32
        s.update({f"blk{l}.{k}": v for k, v in b.items()})
    return s


class Engine:
    """The calls on one engine, as tld_engine.hip makes them: create, then set_gemm_dtype / set_low_latency / finalize in any order; a refused call changes nothing."""

    def __init__(self, cfg, max_batch, env=None, cus=256, device_id=0, ndev=1):
        self.refusal = config_check(cfg, max_batch, device_id, ndev)
        if self.refusal:
            return
        self.sh, self.sw, self.max_batch, self.cus = shape(cfg), switches(env), max_batch, cus
        self.finalized, self.splitk_slices = None, 0
        self.p = plan(self.sh, self.sw, False, 0, max_batch, cus)

    def set_gemm_dtype(self, dtype):
        if self.finalized is not None:
            return "(state) the GEMM operand type must be chosen before tld_engine_finalize_weights"
        r = dtype_refusal(self.sh, dtype, self.p.cls)
        if not r:
            if dtype == 1:      # kept as it was: (1) writes the three switches off and (0) does not put them back
                self.sw.fold_ln1 = self.sw.fold_ln3 = self.sw.fuse_dwconv = False
            self.p = plan(self.sh, self.sw, dtype == 1, self.p.cls, self.max_batch, self.cus)
        return r

    def set_low_latency(self, cls):
        r = class_refusal(self.sh, self.max_batch, cls, self.p.fp8)
        if not r:
            self.splitk_slices = {0: self.splitk_slices, 1: 4, 2: 8}[cls]
            self.p = plan(self.sh, self.sw, self.p.fp8, cls, self.max_batch, self.cus, self.finalized)
        return r

    def finalize(self):
        self.finalized = self.p
        return ""

    def op(self, op):
        return self.finalize() if op == "F" else self.set_gemm_dtype(int(op[1:])) if op[0] == "d" else self.set_low_latency(int(op[1:]))

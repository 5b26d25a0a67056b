"""The host decisions of the training step (csrc/tld_train_plan.h), restated: the derived shape, the workspace, the weight-gradient
split, the ladders of the dispatch sites, the attention backward's dispatch and the launch-path mask a debug step reports.

The weight-gradient split is restated as the TWO loops and the power-of-two ``while`` the engine had before the header gave them one chooser, so that
tests/test_train_plan_host.py holds the chooser against what the step chose then.  block_waves and dispatch are the restatement
tests/test_gpu_attn_bwd_classes.py has always used (it imports them from here)."""
from types import SimpleNamespace as NS

TRANSPOSE_MARGIN = 4096
# launch-path bits: the table in include/tld_hip.h (Trainer.PATH_NAMES has the same order)
(RESID_Q4, RESID_GEN, LNB_Q4, LNB_GEN, EMB_LDS, EMB_PLAIN, TAIL4_16, TAIL4_32, TAIL4_64, TAIL_GEN, TALL_COLS, TALL_PART, COLSUM4, COLSUM, DW_FUSED, DW_UNFUSED, WG_TN,
 WG_TR1, WG_TRSK, WG_PAD, ATT_ONE, ATT_TWO, ATT_MASKED) = (0, 4, 5, 8, 9, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30)
# groups of bits of which a step sets exactly one.  The first seven by construction (one form per engine or per step); the column sums at every configuration
# the tests run (a patch_dim that is no multiple of 4 at 4096 rows or more would set both).  The weight gradients are chosen per product: see WGRAD_SETS.
EXCLUSIVE = {"resid_ln": range(0, 5), "ln_bwd": range(5, 9), "embed": range(9, 14), "tail_dx": range(14, 18), "tall_dw": range(18, 20), "depthwise backward": range(22, 24),
             "attention backward": range(28, 30), "colsum": range(20, 22)}
# the sets of weight-gradient bits a step can show: the untransposed form takes all four products or none (d a multiple of 256), the zero-padded form all four
# (M no multiple of 64); the transposing form splits per product -- d = 128 at 8192 rows cuts the up-projection's product (512 x 128) in 8 and leaves the others whole
WGRAD_SETS = ({WG_TN}, {WG_PAD}, {WG_TR1}, {WG_TRSK}, {WG_TR1, WG_TRSK})


def _get(cfg, name):
    return cfg[name] if isinstance(cfg, dict) else getattr(cfg, name)


def _ceil(a, b):
    return -(-a // b)


def shape(cfg, max_batch):
    d, G = _get(cfg, "embed_dim"), _get(cfg, "image_size") // _get(cfg, "patch_size")
    return NS(d=d, L=_get(cfg, "n_layers"), H=d // 64, G=G, N=G * G, pd=_get(cfg, "n_channels") * _get(cfg, "patch_size") ** 2, hid=d * _get(cfg, "mlp_multiplier"),
              S=_get(cfg, "image_size"), C=_get(cfg, "n_channels"), ne=_get(cfg, "noise_embed_dims"), text=_get(cfg, "text_emb_size"), max_batch=max_batch)


def dw_fused(sh):
    return sh.G <= 16 and sh.N >= 176 and sh.hid % 64 == 0


def workspace(sh):
    """tld_train_create's alloc_all as it was."""
    B, M, d, hid, pd = sh.max_batch, sh.max_batch * sh.N, sh.d, sh.hid, sh.pd
    wide = max(hid, 3 * d)
    need = max(_ceil(M, 256) * 2 * wide, _ceil(M, 32) * 2 * d, B * sh.G * 10 * hid, _ceil(M, 64) * wide, _ceil(M, 64) * pd * d)
    return NS(part_floats=need, splitk_floats=8 * wide * d, tr_rows=M + TRANSPOSE_MARGIN, zero_bias=max(3 * hid, 4096), attn_stats=2 * M * sh.H, scr=pd * d + 64)


# ---- the weight-gradient split, as the two loops and the while loop it was ------------------------------------------------------------------------------------
def _score(M, c, mp, per, cus):
    tiles = per * c
    rounds = _ceil(tiles, cus)
    return tiles / (rounds * cus) * (M / (c * mp))


def untransposed_split(M, Nout, Kin, cus, slice_floats):
    """wgrad_tn: runs padded to 64 rows, c from 1.  None: the kernel does not take the shape."""
    if Nout % 256 or Kin % 256 or M % 64 or M <= 0:
        return None
    per = (Nout // 256) * (Kin // 256)
    best, bsk, bms = 0.0, 1, M
    for c in range(1, 33):
        mp = _ceil(_ceil(M, c), 64) * 64
        if (c > 1 and mp < 1024) or (c - 1) * mp >= M:
            continue
        if c > 1 and c * Nout * Kin > slice_floats:
            continue
        eff = _score(M, c, mp, per, cus)
        if eff > best + 1e-9:
            best, bsk, bms = eff, c, mp
    return bsk, bms


def pow2_split(M, Nout):
    sk = 1
    if Nout % 256 == 0:
        while sk < 8 and (M // (sk * 2)) % 128 == 0 and M // (sk * 2) >= 1024:
            sk *= 2
    return sk, M // sk


def transposing_split(M, Nout, Kin, cus, slice_floats, tr_rows):
    """weight_grad: the power-of-two loop, then runs padded to 128 rows, c from 2, at 4096 rows or more."""
    sk, ms = pow2_split(M, Nout)
    if Nout % 256 == 0 and Kin % 256 == 0 and M % 64 == 0 and M >= 4096:
        per = (Nout // 256) * (Kin // 256)
        best, bsk, bms = 0.0, 0, 0
        for c in range(2, 33):
            mp = _ceil(_ceil(M, c), 128) * 128
            if mp < 1024 or (c - 1) * mp >= M:
                continue
            if c * Nout * Kin > slice_floats or c * mp > tr_rows:
                continue
            eff = _score(M, c, mp, per, cus)
            if eff > best + 1e-9:
                best, bsk, bms = eff, c, mp
        if bsk:
            sk, ms = bsk, bms
    return sk, ms


def wgrad(M, Nout, Kin, cus, tn_wgrad, slice_floats, tr_rows):
    """(path bit of the form, sk, run_rows) of one product, as weight_grad went through its branches."""
    if tn_wgrad:
        s = untransposed_split(M, Nout, Kin, cus, slice_floats)
        if s:
            return (WG_TN, *s)
    sk, ms = transposing_split(M, Nout, Kin, cus, slice_floats, tr_rows)
    if M % 64:
        assert sk == 1, (M, Nout, sk)          # (M a multiple of 16: a halving that passes needs M a multiple of 256)
        return WG_PAD, 1, _ceil(M, 64) * 64
    return (WG_TR1 if sk == 1 else WG_TRSK), sk, ms


# ---- the attention backward ---------------------------------------------------------------------------------------------------------------------------------------
def block_waves(n):
    """attn_bwd_block_waves: waves per workgroup (block width 32 nw) at n tokens."""
    if n <= 256:
        return (n + 31) // 32
    best, pad = 8, 1 << 30
    for nw in (8, 7, 6, 5, 4):
        npad = -(-n // (32 * nw)) * 32 * nw
        if nw == 7 and npad != n:
            continue
        if npad < pad:
            pad, best = npad, nw
    return best


def dispatch(n):
    """launch_bwd: (mode, NW, masked) at n tokens, mode "fused" (one workgroup per (sample, head)) or "two" (dQ kernel + dK / dV kernel)."""
    if n in (64, 128, 256):
        return "fused", n // 32, False
    if n > 256 and n % 256 == 0:
        return "two", 8, False
    nw = block_waves(n)
    return ("fused" if n < 256 else "two"), nw, n % (32 * nw) != 0


def attn_dispatch(n, has_stats=True):
    """attn_bwd_dispatch: (mode 0 refused | 1 one kernel | 2 two kernels, waves, masked)."""
    if n <= 0 or n % 16 or (n > 256 and not has_stats):
        return 0, 0, False
    mode, nw, masked = dispatch(n)
    return (1 if mode == "fused" else 2), nw, masked


# ---- the plan of one step ---------------------------------------------------------------------------------------------------------------------------------------
def step_plan(sh, ws, batch, cus, tn_wgrad):
    d, hid, pd, G, N = sh.d, sh.hid, sh.pd, sh.G, sh.N
    M = batch * N
    bits = set()
    p = NS(batch=batch, M=M)
    if pd * d * 4 <= 65536:
        p.embed_lds = 1 if d <= 256 else 2 if d <= 512 else 3 if d <= 768 else 4
        p.embed_wgs = min(_ceil(M, 4), 4 * cus)
        bits.add(EMB_LDS + p.embed_lds - 1)
    else:
        p.embed_lds, p.embed_wgs = 0, _ceil(M, 4)
        bits.add(EMB_PLAIN)
    p.resid_q4 = {256: 1, 512: 2, 768: 3, 1024: 4}.get(d, 0)
    bits.add(RESID_Q4 + p.resid_q4 - 1 if p.resid_q4 else RESID_GEN)
    p.lnb_q4 = {256: 1, 512: 2, 768: 3}.get(d, 0)
    bits.add(LNB_Q4 + p.lnb_q4 - 1 if p.lnb_q4 else LNB_GEN)
    p.tail4 = pd if pd in (16, 32, 64) else 0
    bits.add({16: TAIL4_16, 32: TAIL4_32, 64: TAIL4_64}.get(pd, TAIL_GEN))
    p.tall = []
    for K in (d, d, pd):              # dWout, the embedding's linear, its convolution
        cols = pd in (16, 32, 64) and _ceil(M, 64) * pd * K <= ws.part_floats
        p.tall.append([pd if cols else 0, K, (_ceil(M, 64) if cols else _ceil(M, 256)) * pd * K])
        bits.add(TALL_COLS if cols else TALL_PART)
    p.dw_fused = int(dw_fused(sh))
    bits.add(DW_FUSED if p.dw_fused else DW_UNFUSED)
    p.dw_rows = min(G, 16)
    p.dw_grid = batch * (hid // 64) * _ceil(G, p.dw_rows)
    p.dw_lds = min(p.dw_rows + 2, G) * G * 128
    p.dw_bwd_grid, p.dw_bwd_lds = (batch * (hid // 64), 2 * N * 128) if p.dw_fused else (0, 0)
    p.colsum = []
    for k, cols in enumerate((pd, d, hid)):      # out_proj / conv bias; down / linear bias; up bias (the fused depthwise backward sums that one itself)
        used = k != 2 or not p.dw_fused
        four = cols % 4 == 0 and M >= 4096
        p.colsum.append([int(used), int(four), cols, _ceil(M, 64 if four else 256) * cols])
        if used:
            bits.add(COLSUM4 if four else COLSUM)
    p.wg = [list(wgrad(M, a, b, cus, tn_wgrad, ws.splitk_floats, ws.tr_rows)) for a, b in ((d, hid), (hid, d), (d, d), (3 * d, d))]
    bits.update(w[0] for w in p.wg)
    mode, nw, masked = attn_dispatch(N)
    p.attn = [mode, nw, int(masked)]
    bits.add(ATT_ONE if mode == 1 else ATT_TWO)
    if masked:
        bits.add(ATT_MASKED)
    p.paths = sum(1 << b for b in bits)
    demands = [["ln_bwd", _ceil(M, 32) * 2 * d], ["ln_bwd cond", _ceil(2 * batch, 32) * 2 * d], ["ln_small_bwd", _ceil(M, 256) * 2 * pd],
               ["depthwise backward", batch * 11 * hid if p.dw_fused else batch * G * 10 * hid]]
    demands += [[n, t[2]] for n, t in zip(("tall_dw out_proj", "tall_dw linear", "tall_dw conv"), p.tall)]
    demands += [[n, c[3]] for n, c in zip(("colsum pd", "colsum d", "colsum hid"), p.colsum) if c[0]]
    return p, demands


def expected_mask(config, batch, max_batch, cus, tn_wgrad):
    """The mask tld_train_debug_paths reports after a debug step of `batch` samples on an engine of `max_batch`."""
    sh = shape(config, max_batch)
    return step_plan(sh, workspace(sh), batch, cus, bool(tn_wgrad))[0].paths

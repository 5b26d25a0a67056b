"""CPU: the mode of an inference engine -- csrc/tld_body_plan.h through tests/host/body_plan_main.cpp, built by the host compiler
plain and under AddressSanitizer + UBSan, against the restatement in tests/body_plan_ref.py; the cross-checks between what a plan takes, what it holds and
what it reserves; and every refusal of tld_engine_create, tld_engine_set_low_latency and tld_engine_set_gemm_dtype that is arithmetic on the configuration,
with its full text and its precedence."""
import itertools
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import pytest

import body_plan_ref as B
import test_gpu_forward_stages as FS
import test_gpu_fp8_stages as F8
from conftest import cfg_from_arr, load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("image_size", "noise_embed_dims", "patch_size", "embed_dim", "n_layers", "text_emb_size", "n_channels", "mlp_multiplier")


def _cfg(d=768, image=32, blocks=2, patch=2, C=4, mult=4, ne=256, text=768):
    return NS(image_size=image, noise_embed_dims=ne, patch_size=patch, embed_dim=d, n_layers=blocks, text_emb_size=text, n_channels=C, mlp_multiplier=mult)


def _line(name, cfg, max_batch, ops="-", env=None, cus=256, device_id=0, ndev=1):
    return " ".join([name.replace(" ", "_"), *(str(getattr(cfg, f)) for f in FIELDS), str(max_batch), str(device_id), str(ndev), str(cus), ops,
                     *(f"{k}={v}" for k, v in (env or {}).items())])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver, built twice (run directly, nothing preloaded); ``run(lines)`` returns the parsed output, the same from both builds."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    tmp = tmp_path_factory.mktemp("body_plan")
    src = [os.path.join(REPO, "tests", "host", "body_plan_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"body_plan_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exes[tag]], check=True)

    def run(lines):
        path = tmp / f"cases_{len(os.listdir(tmp))}.txt"
        path.write_text("".join(ln + "\n" for ln in lines))
        outs = []
        for tag, exe in exes.items():
            r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
            assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
            outs.append(r.stdout)
        assert outs[0] == outs[1], "the sanitizer build answers differently"
        res = [json.loads(ln) for ln in outs[0].splitlines()]
        assert len(res) == len(lines)
        return res

    return run


# ---- the sweep: every configuration the GPU stage tests and the g16 golden sweep run, crossed with every input of the plan -------------------------------------
def _configs():
    out = {}
    for name, (kw, _, max_batch, _, _) in FS.CASES.items():
        out["fwd " + name] = (NS(**kw), max_batch)
    out["fwd fp8 path"] = (NS(**FS.FP8_PATH_CASE[0]), FS.FP8_PATH_CASE[1])
    for name, (kw, _, max_batch, _) in F8.CASES.items():
        out["fp8 " + name] = (NS(**kw), max_batch)
    g = load_golden("g16_config_sweep.npz")
    for tag in g["tags"]:
        out[f"g16 {tag}"] = (cfg_from_arr(g[f"{tag}_cfg"]), 2)
    assert len(g["tags"]) == 25
    return out


ENVS = [{}] + [{k: "0"} for k in B.SWITCHES] + [{k: "0" for k in B.SWITCHES}]


def _sweep():
    for (name, (cfg, max_batch)), env, pair, dtype, cls, cus in itertools.product(_configs().items(), ENVS, "012", (0, 1), (0, 1, 2), (256, 304)):
        yield name, cfg, max_batch, dict(env, TLD_QKV_ATTN_PAIR=pair), f"d{dtype},c{cls}", cus


def _check_against_ref(o, cfg, max_batch, env, ops, cus, **kw):
    """One line of the driver against the restatement: refusals, shape, switches, plan, image table; returns (engine of the restatement, the driver's plan)."""
    e = B.Engine(cfg, max_batch, env, cus, **kw)
    assert o["create"] == e.refusal
    if e.refusal:
        return e, None
    assert o["ops"] == [e.op(op) for op in ops.split(",") if op != "-"]
    assert o["shape"] == vars(e.sh)
    assert o["switches"] == {k: int(v) for k, v in vars(e.sw).items()}
    assert o["plan"] == {k: int(v) for k, v in vars(e.p).items()}
    p = NS(**o["plan"])
    assert o["pair_launch"] == "".join(str(int(B.pair_launch(p, b))) for b in range(1, max_batch + 1))
    ref = B.images(e.sh, p)
    assert [r[0] for r in o["images"]] == list(dict.fromkeys(r[0] for r in o["images"])) and {r[0] for r in o["images"]} == set(ref)
    for member, name, dtype, numel, margin, held in o["images"]:
        assert (name, dtype, numel, margin, int(held)) == tuple(int(v) if isinstance(v, bool) else v for v in ref[member]), member
    return e, p


def _check_invariants(o, e, p, max_batch):
    """What the engine's own code could not check: the plan's three faces agree."""
    sh = e.sh
    held = {r[0] for r in o["images"] if r[5]}
    missing = B.reads(sh, p, max_batch) - held
    assert not missing, f"a taken path reads images the plan does not hold: {sorted(missing)}"
    assert bool(p.seam) == bool(p.fuse_dw and sh.grid == 32)
    for producer, quant in ((p.ln_mx8, p.quant_qkv), (p.cross_mx8, p.quant_up), (p.dw_mx8, p.quant_down)):
        assert (producer != quant) if p.fp8 else (not producer and not quant)
    assert (not p.pair or p.pair_held) and (not p.pair_held or p.fused_qa or e.finalized is not None) and (not p.fold_tail or p.fold_tail_held)
    assert not (p.fold_tail and p.ll_split) and not (p.fp8 and (p.ll_split or p.fold_tail or p.fused_qa or p.fuse_dw or p.fold_ln1 or p.fold_ln3))
    for b in range(1, max_batch + 1):          # a slot for every workgroup of every pair launch
        assert not B.pair_launch(p, b) or min(b * (sh.H // 2), p.cus) <= p.pair_slots
    reserved, taken = dict(map(tuple, o["stages"])), B.snapped(sh, p, max_batch)
    assert len(reserved) == len(o["stages"])
    if p.fold_tail_held and not p.fold_tail:      # THE exception, kept: a low-latency engine that holds the fold image reserves the last "mlp" at 4 bytes per element
        last = f"blk{sh.L - 1}.mlp"
        assert reserved[last] == max_batch * sh.ntok * sh.d * 4 and taken[last] == reserved[last] // 2
        taken[last] = reserved[last]
    if e.splitk_slices and not p.ll_split:        # (only a class set and cleared again: the buffer outlives its class, and so does its stage)
        taken.update({f"blk{l}.splitk": e.splitk_slices * max_batch * sh.ntok * sh.d * 4 for l in range(sh.L)})
    assert reserved == taken, (sorted(set(reserved) ^ set(taken)), [k for k in reserved if k in taken and reserved[k] != taken[k]])


def test_sweep_against_the_restatement_and_invariants(driver):
    cases = list(_sweep())
    assert len(cases) == 55 * 8 * 3 * 2 * 3 * 2
    outs = driver([_line(name, cfg, mb, ops, env, cus) for name, cfg, mb, env, ops, cus in cases])
    seen = set()
    for o, (name, cfg, mb, env, ops, cus) in zip(outs, cases):
        e, p = _check_against_ref(o, cfg, mb, env, ops, cus)
        assert p is not None, (name, o["create"])
        _check_invariants(o, e, p, mb)
        seen.add((p.fp8, p.cls, p.fold_ln1, p.fold_ln3, p.fused_qa, p.pair, p.fuse_dw, p.seam, p.fold_tail, p.ln_mx8, p.cross_mx8, p.dw_mx8))
        seen.update(f"refused: {r[:24]}" for r in o["ops"] if r)
    # the sweep reaches every path and both kinds of setter refusal that depend on the shape
    for k, name in enumerate(("fp8", "cls", "fold_ln1", "fold_ln3", "fused_qa", "pair", "fuse_dw", "seam", "fold_tail", "ln_mx8", "cross_mx8", "dw_mx8")):
        assert {bool(s[k]) for s in seen if isinstance(s, tuple)} == {False, True}, name
    assert {s for s in seen if isinstance(s, str)} >= {"refused: low-latency class: bf16 ", "refused: low-latency class 1: eng", "refused: low-latency class 2: eng",
                                                        "refused: low-latency class: needs", "refused: fp8 GEMMs need embed_dim"}


def test_the_defaults_of_the_flagship(driver):
    """C1 by name: the 100M model at the bench batch takes every fused path, holds the pair images and no seam."""
    cfg, mb = NS(**FS.CASES["C1"][0]), FS.CASES["C1"][2]
    o, = driver([_line("C1", cfg, mb)])
    want = dict(fp8=0, cls=0, fold_ln1=1, fold_ln3=1, fused_qa=1, pair_held=1, pair=1, pair_always=0, pair_slots=256, fuse_dw=1, seam=0, fold_tail_held=1, fold_tail=1,
                ln_mx8=0, cross_mx8=0, dw_mx8=0, quant_qkv=0, quant_up=0, quant_down=0, ll_split=0, share_l0=1, guidance_skip=1, heads=12, cus=256)
    assert o["plan"] == want
    assert o["pair_launch"][127] == "1" and o["pair_launch"][63] == "0"      # blocks 1 - 11 of C1 take pairs, block 0 on the shared half batch does not


# ---- sequences of calls: what is held is frozen at finalize ---------------------------------------------------------------------------------------------------
SEQUENCES = {
    "class before finalize, cleared after": ("c1,F,c0", dict(pair_held=0, pair=0, fused_qa=1, fold_tail=1, ll_split=0)),
    "class after finalize": ("F,c1", dict(pair_held=1, pair=0, fused_qa=1, fold_tail_held=1, fold_tail=0, ll_split=4)),
    "class 2 after finalize, then 1": ("F,c2,c1", dict(pair_held=1, pair=0, ll_split=4)),
    "class set and cleared": ("c2,c0,F", dict(pair_held=1, pair=1, ll_split=0, fold_tail=1)),
    "dtype 1 then 0": ("d1,d0,F", dict(fp8=0, fold_ln1=0, fold_ln3=0, fused_qa=0, pair_held=0, fuse_dw=0, fold_tail_held=1, fold_tail=1)),
    "dtype after finalize": ("F,d1", dict(fp8=0, fold_ln1=1)),
}


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_call_sequences(driver, name):
    ops, want = SEQUENCES[name]
    cfg, mb, env = _cfg(768, 32, 2), 4, {"TLD_QKV_ATTN_PAIR": "2"}      # (2: at 1 no engine inside a low-latency class's capacity has a batch that takes pairs)
    o, = driver([_line(name, cfg, mb, ops, env)])
    e, p = _check_against_ref(o, cfg, mb, env, ops, 256)
    _check_invariants(o, e, p, mb)
    assert {k: o["plan"][k] for k in want} == want
    if name == "dtype 1 then 0":      # the corner kept on purpose: (1) wrote three switches off, (0) did not put them back
        assert {k: o["switches"][k] for k in ("fold_ln1", "fold_ln3", "fuse_dwconv", "fold_tail", "fuse_qkv_attn")} == dict(fold_ln1=0, fold_ln3=0, fuse_dwconv=0, fold_tail=1,
                                                                                                                            fuse_qkv_attn=1)
        assert {r[0] for r in o["images"] if r[5]} >= {"qkv_w", "up_w", "down_w"}
    if name == "dtype after finalize":
        assert o["ops"] == ["", "(state) the GEMM operand type must be chosen before tld_engine_finalize_weights"]
    if name == "class set and cleared":
        assert dict(map(tuple, o["stages"]))["blk0.splitk"] == 8 * mb * 256 * 768 * 4


# ---- the switches ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env,want", [
    ({}, dict(fold_ln1=1, fold_ln3=1, fold_tail=1, fuse_dwconv=1, fuse_qkv_attn=1, fp8_fused=1, qkv_pair=1, share_l0=1, guidance_skip=1)),
    ({"TLD_FOLD_LN1": "on"}, dict(fold_ln1=0)),                       # no number: atoi gives 0, which is off
    ({"TLD_FOLD_LN3": "", "TLD_FUSE_DWCONV": "-1", "TLD_FOLD_TAIL": "00", "TLD_FP8_FUSED": "2x", "TLD_FUSE_QKV_ATTN": "+0"},
     dict(fold_ln3=0, fuse_dwconv=1, fold_tail=0, fp8_fused=1, fuse_qkv_attn=0)),
    ({"TLD_QKV_ATTN_PAIR": "7"}, dict(qkv_pair=2)), ({"TLD_QKV_ATTN_PAIR": "-3"}, dict(qkv_pair=0)), ({"TLD_QKV_ATTN_PAIR": "x"}, dict(qkv_pair=0)),
    ({"TLD_SHARE_L0": "0", "TLD_GUIDANCE_SKIP": "0"}, dict(share_l0=0, guidance_skip=0)),
])
def test_switches(driver, env, want):
    cfg = _cfg()
    o, = driver([_line("switches", cfg, 4, "-", env)])
    _check_against_ref(o, cfg, 4, env, "-", 256)
    assert {k: o["switches"][k] for k in want} == want


# ---- refusals: each reached once with its full text, each in front of the one below it -----------------------------------------------------------------------
# (config, max_batch, device_id, text).  Every row but the last also breaks the rule of the row BELOW it, so its text shows its precedence.
# "hidden width must be a multiple of 64" cannot be reached: embed_dim is a multiple of 64 by then, and the hidden width a multiple of embed_dim.
CREATE = [
    (_cfg(d=700, patch=0), 4, 0, "embed_dim=700 unsupported: must be a multiple of the head width 64 (n_heads = embed_dim // 64, tld/transformer_blocks.py:126-128) and <= 1024 "
                                 "(the row kernels hold a token row in 8 x 128-feature register groups)"),
    (_cfg(image=30, patch=4), 4, 0, "image_size=30 must be divisible by patch_size=4"),      # (7.5 squared is no multiple of 16 either)
    (_cfg(image=6, patch=1, C=80), 4, 0, "token count 36 unsupported: image_size / patch_size must be a multiple of 4"),
    (_cfg(image=32, patch=4, C=8, ne=3), 4, 0, "patch_dim=128 > 64 unsupported"),
    (_cfg(ne=3, blocks=0), 4, 0, "noise_embed_dims must be even"),
    (_cfg(blocks=0, image=256), 171, 0, "non-positive size in config"),
    (_cfg(image=256), 171, 5, "max_batch=171: the hidden activation (17213423616 bytes) must stay below 4 GiB; run larger batches as several calls"),
    (_cfg(d=1024, image=16, patch=4), 4, 5, "device_id 5 out of range (1 devices)"),
    (_cfg(d=1024, image=16, patch=4), 4, 0, "embed_dim=1024 with patch_dim=64 needs 278528 / 262144 / 73792 bytes of LDS in the embed / out-proj / cross-attention row kernels "
                                            "(limit 163840 each): reduce patch_size*patch_size*n_channels or embed_dim"),
]
MENDS = [dict(embed_dim=768), dict(image_size=28), dict(image_size=8), dict(n_channels=4), dict(noise_embed_dims=256), dict(n_layers=2), dict(max_batch=4), dict(device_id=0)]
KEYS = ["embed_dim=", "must be divisible", "token count", "patch_dim=", "noise_embed_dims", "non-positive", "hidden activation", "device_id", "of LDS"]
MORE_CREATE = [(_cfg(d=0), 4, 0, "embed_dim=0 unsupported"), (_cfg(d=1088), 4, 0, "embed_dim=1088 unsupported"), (_cfg(ne=0), 4, 0, "noise_embed_dims must be even"),
               (_cfg(ne=-2), 4, 0, "noise_embed_dims must be even"), (_cfg(), 0, 0, "non-positive size in config"), (_cfg(mult=0), 4, 0, "non-positive size in config"),
               (_cfg(text=0), 4, 0, "non-positive size in config"), (_cfg(), 4, -1, "device_id -1 out of range (1 devices)"), (_cfg(), 4, 1, "device_id 1 out of range (1 devices)")]


def test_create_refusals(driver):
    rows = CREATE + MORE_CREATE
    outs = driver([_line(f"create{k}", cfg, mb, device_id=dev) for k, (cfg, mb, dev, _) in enumerate(rows)])
    for k, (o, (cfg, mb, dev, text)) in enumerate(zip(outs, rows)):
        assert o["create"] == text if k < len(CREATE) else o["create"].startswith(text), (k, o["create"])
        assert o["create"] == B.config_check(cfg, mb, dev, 1) and set(o) == {"name", "create"}
    for k, ((cfg, mb, dev, _), mend) in enumerate(zip(CREATE, MENDS)):      # with its own fault mended, a row shows the text of the row below: it broke both rules
        fixed = {**vars(cfg), "max_batch": mb, "device_id": dev, **mend}
        mb2, dev2 = fixed.pop("max_batch"), fixed.pop("device_id")
        assert KEYS[k + 1] in B.config_check(NS(**fixed), mb2, dev2, 1), (k, mend)


# ---- the 32-bit reach: the exact boundary of max_batch, and no accepted engine whose forward launch_gemm would refuse -------------------
# (config, the largest max_batch create accepts, the words of the refusal one beyond it).  The hidden activation binds from mlp_multiplier 2 on (at 2 q|k is as
# large); at 1 q|k [M, 2 d] is twice the hidden activation and binds.  The last two: narrow rows, where the hidden-activation rule alone would admit 2^25 rows
# -- beyond the 24-bit row factor of the GEMM tile DMA -- and 524 288 samples of 16 tokens, beyond the z axis of the attention kernels' grid.
REACH = [
    (_cfg(d=768, image=32, mult=4), 2730, "the hidden activation (4295491584 bytes)"),
    (_cfg(d=768, image=64, mult=4), 682, "the hidden activation (4297064448 bytes)"),
    (_cfg(d=768, image=128, mult=4), 170, "the hidden activation (4303355904 bytes)"),
    (_cfg(d=256, image=32, mult=4), 8191, "the hidden activation (4294967296 bytes)"),
    (_cfg(d=384, image=32, patch=1, C=8, mult=2), 2730, "the hidden activation (4295491584 bytes)"),
    (_cfg(d=768, image=32, mult=2), 5461, "the hidden activation (4295491584 bytes)"),
    (_cfg(d=768, image=32, mult=1), 5461, "the q|k activation (max_batch x tokens x 2 embed_dim x 2 B = 4295491584 bytes)"),
    (_cfg(d=512, image=64, mult=1), 2047, "the q|k activation (max_batch x tokens x 2 embed_dim x 2 B = 4294967296 bytes)"),
    (_cfg(d=64, image=32, mult=1), 65535, "the q|k activation (max_batch x tokens x 2 embed_dim x 2 B = 4294967296 bytes)"),
    (_cfg(d=64, image=8, mult=1), 65535, "the self-attention kernels put one sample on each block of the grid's z axis (at most 65535)"),
]


def _fp8_ok(cfg):
    return cfg.embed_dim % 128 == 0 and (cfg.embed_dim * cfg.mlp_multiplier) % 128 == 0


def test_reach_boundary_of_max_batch(driver):
    """The largest accepted max_batch and one more, mlp_multiplier 1, 2 and 4: the refusal names the buffer and, for the rules of section 7.19, the largest max_batch
    that fits; the accepted engine takes the fp8 mode where its widths allow (a8 [M, hid] bytes, its scales and the seam buffer are smaller than the hidden activation:
    no rule of their own), and launch_gemm's reach check passes for every GEMM of its forward with bf16 and with fp8 operands."""
    lines = []
    for k, (cfg, mb, _) in enumerate(REACH):
        lines += [_line(f"reach{k} in", cfg, mb, "d1" if _fp8_ok(cfg) else "-"), _line(f"reach{k} out", cfg, mb + 1)]
    outs = driver(lines)
    for k, (cfg, mb, words) in enumerate(REACH):
        good, bad = outs[2 * k], outs[2 * k + 1]
        assert good["create"] == "" == B.config_check(cfg, mb), (k, good["create"])
        assert good["ops"] == ([""] if _fp8_ok(cfg) else []) and good["plan"]["fp8"] == int(_fp8_ok(cfg))
        assert [g[0] for g in good["gemm_reach"]] == ["QKV projection", "up-projection", "down projection"]
        assert all(g[1] == 1 and g[2] == 1 for g in good["gemm_reach"]), (k, good["gemm_reach"])
        assert mb * good["shape"]["ntok"] <= 1 << 24
        assert bad["create"] == B.config_check(cfg, mb + 1) and words in bad["create"], (k, bad["create"])
        assert bad["create"].startswith(f"max_batch={mb + 1}: ") and "run larger batches as several calls" in bad["create"]
        if "hidden activation" not in words:
            assert f"the largest max_batch that fits is {mb};" in bad["create"], bad["create"]
    # the figures of the issue's table: 2730 / 682 / 170 at d 768, 8190 < 8191 at d 256
    assert [r[1] for r in REACH[:4]] == [2730, 682, 170, 8191]


def test_no_accepted_engine_is_refused_by_launch_gemm(driver):
    """At the largest max_batch create accepts, for every width, grid and multiplier the engine takes: every GEMM of the forward is inside launch_gemm's reach (a
    create that accepts must not be followed by a refusal in the middle of a forward)."""
    cases = []
    for d in range(64, 1025, 64):
        for image, patch in ((8, 2), (32, 2), (64, 2), (128, 2), (24, 2)):
            for mult in (1, 2, 3, 4, 8):
                cfg = _cfg(d=d, image=image, patch=patch, mult=mult)
                lo, hi = 1, 1 << 21                      # bisect the boundary on the restatement (monotone in max_batch)
                while lo < hi:
                    mid = (lo + hi + 1) // 2
                    lo, hi = (mid, hi) if "max_batch=" not in B.config_check(cfg, mid) else (lo, mid - 1)
                cases.append((cfg, lo))
    outs = driver([_line(f"fit{k}", cfg, mb) for k, (cfg, mb) in enumerate(cases)] + [_line(f"over{k}", cfg, mb + 1) for k, (cfg, mb) in enumerate(cases)])
    n = len(cases)
    for k, (cfg, mb) in enumerate(cases):
        o, over = outs[k], outs[n + k]
        if o["create"]:                                  # (refused for another reason -- the LDS of the row kernels at d = 1024 -- at every max_batch)
            assert "max_batch=" not in o["create"]
            continue
        assert all(g[1] == 1 and g[2] == 1 for g in o["gemm_reach"]), (vars(cfg), mb, o["gemm_reach"])
        assert over["create"].startswith(f"max_batch={mb + 1}: "), (vars(cfg), mb, over["create"])


# (config, max_batch, ops, the refusal of each op).  Of two faults the upper one is reported.
SETTERS = [
    (_cfg(), 4, "c3", ["low-latency class 3: 0 = off, 1 = four K-splits (engines up to 4096 token rows), 2 = eight (up to 1024)"]),
    (_cfg(), 4, "d1,c3", ["", "low-latency class 3: 0 = off, 1 = four K-splits (engines up to 4096 token rows), 2 = eight (up to 1024)"]),       # range before fp8
    (_cfg(), 20, "d1,c1", ["", "low-latency class: bf16 GEMM operands only -- this engine runs MX-fp8 GEMMs (tld_engine_set_gemm_dtype), whose down projection has no split-K form"]),      # fp8 before capacity
    (_cfg(d=256), 20, "c1", ["low-latency class 1: engine capacity 5120 token rows (max_batch 20 x 256 tokens) exceeds 4096 -- at that size the default tiles fill the chip"]),      # capacity before widths
    (_cfg(), 6, "c2,c1", ["low-latency class 2: engine capacity 1536 token rows (max_batch 6 x 256 tokens) exceeds 1024 -- at that size class 1 (four K-splits) is the faster one", ""]),
    (_cfg(d=256), 4, "c1", ["low-latency class: needs embed_dim 384 or 768 (got 256) and a hidden width that splits into 4 multiples of 64 (got 1024)"]),
    (_cfg(d=384, mult=1), 2, "c1,c2", ["low-latency class: needs embed_dim 384 or 768 (got 384) and a hidden width that splits into 4 multiples of 64 (got 384)",
                                       "low-latency class: needs embed_dim 384 or 768 (got 384) and a hidden width that splits into 8 multiples of 64 (got 384)"]),
    (_cfg(d=384, mult=2), 2, "c1,c2", ["", "low-latency class: needs embed_dim 384 or 768 (got 384) and a hidden width that splits into 8 multiples of 64 (got 768)"]),
    (_cfg(), 4, "d2,d-1", ["gemm dtype 2: 0 = bf16, 1 = MX-fp8 (e4m3 + E8M0 block scales)", "gemm dtype -1: 0 = bf16, 1 = MX-fp8 (e4m3 + E8M0 block scales)"]),
    (_cfg(), 4, "c1,d2", ["", "gemm dtype 2: 0 = bf16, 1 = MX-fp8 (e4m3 + E8M0 block scales)"]),       # range before the exclusion
    (_cfg(d=192, image=16), 4, "d1", ["fp8 GEMMs need embed_dim and hidden width multiples of 128"]),
    (_cfg(d=384, mult=1), 4, "d1", [""]),
    (_cfg(d=384, mult=2), 2, "c1,d1,d0,c0,d1", ["", "fp8 GEMMs and the low-latency class exclude each other (the split-K down projection is bf16 only): clear "
                                                     "tld_engine_set_low_latency first", "", "", ""]),      # (d = 384 x 2 = 768: the exclusion, not the widths)
]


def test_setter_refusals(driver):
    outs = driver([_line(f"setter{k}", cfg, mb, ops) for k, (cfg, mb, ops, _) in enumerate(SETTERS)])
    for o, (cfg, mb, ops, texts) in zip(outs, SETTERS):
        assert o["create"] == "" and o["ops"] == texts, (ops, o["ops"])
        e, p = _check_against_ref(o, cfg, mb, None, ops, 256)
        _check_invariants(o, e, p, mb)

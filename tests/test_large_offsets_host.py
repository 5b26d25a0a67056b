"""CPU: the sizes at which the kernels' 32-bit offsets and 16-bit grid axes end, as refusals -- csrc/tld_reach.h through
tests/host/reach_main.cpp, built by the host compiler plain and under AddressSanitizer + UBSan, against the arithmetic written out here; and the same refusals
through the library's own entry points: tld_train_create, tld_clip_create, tld_clip_vis_create and the five raw-buffer hooks refuse BEFORE any HIP call, so a
machine without a device can ask them (only refused sizes are asked: an accepted one would go on to the device).  The inference engine's rules are held by
tests/test_body_plan_host.py; the accepted side of every boundary is executed by tests/test_gpu_large_offsets.py."""
import ctypes as C
import json
import os
import shutil
import subprocess
from types import SimpleNamespace as NS

import pytest

from transformer_latent_diffusion_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TLD_ERR_INVALID = 1
FIELDS = ("image_size", "noise_embed_dims", "patch_size", "embed_dim", "n_layers", "text_emb_size", "n_channels", "mlp_multiplier")
GIB4 = 1 << 32


def _cfg(d=768, image=32, blocks=1, patch=2, C=4, mult=4, ne=256, text=768):
    return NS(image_size=image, noise_embed_dims=ne, patch_size=patch, embed_dim=d, n_layers=blocks, text_emb_size=text, n_channels=C, mlp_multiplier=mult)


def _train_line(cfg, max_batch):
    return " ".join(["train", *(str(getattr(cfg, f)) for f in FIELDS), str(max_batch)])


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """The driver, built twice (run directly, nothing preloaded); ``run(lines)`` returns the parsed output, the same from both builds."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    tmp = tmp_path_factory.mktemp("reach")
    src = [os.path.join(REPO, "tests", "host", "reach_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = {}
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exes[tag] = str(tmp / f"reach_main_{tag}")
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


# ---- the training engine -----------------------------------------------------------------------------------------------------------------------------------------
def train_largest(cfg):
    """The largest max_batch tld_train_create accepts, from the three rules written out: T1 / T2 below 4 GiB; row chunks and (sample, image row) pairs on a y axis."""
    G = cfg.image_size // cfg.patch_size
    N, d = G * G, cfg.embed_dim
    hid = d * cfg.mlp_multiplier
    wide = max(hid, 3 * d)
    t12 = ((GIB4 - 1) // (wide * 2) - 4096) // N                  # (max_batch N + 4096) wide 2 <= 2^32 - 1
    rows = (65535 * 32) // N if N % 64 else (65535 * 64 - 4096) // N
    dw_fused = G <= 16 and N >= 176 and hid % 64 == 0
    return min(t12, rows, 10 ** 9 if dw_fused else 65535 // G), dict(t12=t12, rows=rows, pairs=None if dw_fused else 65535 // G)


# (config, the largest max_batch, words of the refusal one beyond it).  The first three are the sizes tests/test_gpu_large_offsets.py trains at or below.
TRAIN = [
    (_cfg(d=768, image=32), 2714, "the transposed weight-gradient operands T1 / T2 ((max_batch x tokens + 4096) x max(hidden width, 3 embed_dim) x 2 B = 4295491584 bytes)"),
    (_cfg(d=128, image=128), 1022, "the transposed weight-gradient operands T1 / T2"),
    (_cfg(d=768, image=32, mult=1), 3624, "the transposed weight-gradient operands T1 / T2"),       # dqkv [M, 3 d] is the wide one
    (_cfg(d=64, image=128), 1022, "64-row chunks of them and of 4096 rows more on the grid's y axis (at most 65535)"),
    (_cfg(d=64, image=72), 1618, "32-row tiles of them on the grid's y axis (at most 65535)"),
    (_cfg(d=64, image=8), 16383, "one block per sample and image row on the grid's y axis (at most 65535)"),
    (_cfg(d=64, image=40, mult=1), 3276, "one block per sample and image row on the grid's y axis (at most 65535)"),
]


def test_train_create_boundary(driver):
    for cfg, mb, _ in TRAIN:
        assert train_largest(cfg)[0] == mb, (vars(cfg), train_largest(cfg))
    outs = driver([_train_line(cfg, mb + k) for cfg, mb, _ in TRAIN for k in (0, 1)])
    for k, (cfg, mb, words) in enumerate(TRAIN):
        good, bad = outs[2 * k], outs[2 * k + 1]
        assert good["refusal"] == "" and good["unfit"] == 0 and good["untested"] == 0 and good["gemms"] > 16, (k, good)
        assert bad["refusal"].startswith(f"max_batch={mb + 1}: ") and words in bad["refusal"], (k, bad)
        assert f"the largest max_batch that fits is {mb};" in bad["refusal"] and "run larger batches as several calls" in bad["refusal"], bad


def test_no_accepted_trainer_is_refused_by_launch_gemm(driver):
    """At the largest max_batch of every width, grid and multiplier: no GEMM launch of the step -- the linears over M rows and the transposing weight gradient at
    every split count its workspace admits -- lies beyond launch_gemm's reach; and one sample more is refused by create."""
    cases = [_cfg(d=d, image=2 * g, mult=m) for d in range(64, 1025, 64) for g in (4, 12, 16, 20, 32, 64) for m in (1, 2, 3, 4, 8)]
    best = [train_largest(c)[0] for c in cases]
    outs = driver([_train_line(c, b) for c, b in zip(cases, best)] + [_train_line(c, b + 1) for c, b in zip(cases, best)])
    for k, (c, b) in enumerate(zip(cases, best)):
        assert outs[k]["refusal"] == "" and outs[k]["unfit"] == 0 and outs[k]["untested"] == 0, (vars(c), b, outs[k])
        assert outs[len(cases) + k]["refusal"].startswith(f"max_batch={b + 1}: "), (vars(c), b)


def test_train_create_keeps_its_other_refusals(driver):
    rows = [(_cfg(d=700), "embed_dim must be a multiple of 64 (the head width), <= 1024"), (_cfg(image=30, patch=4), "image_size must be a multiple of patch_size"),
            (_cfg(image=20), "the training step supports image_size / patch_size = G with G a multiple of 4, 4 <= G <= 64 (16 .. 4096 tokens); got G = 10"),
            (_cfg(image=32, patch=4, C=8), "patch_dim must be <= 64"), (_cfg(ne=3), "bad configuration"), (_cfg(blocks=0), "bad configuration")]
    outs = driver([_train_line(c, 4) for c, _ in rows] + [_train_line(_cfg(), 0)])
    assert [o["refusal"] for o in outs] == [t for _, t in rows] + ["bad configuration"]


def test_train_create_refuses_through_the_library_before_any_hip_call():
    L = _lib.lib()
    for cfg, mb, words in TRAIN:
        h = C.c_void_p()
        c = _lib.TldConfig(*(getattr(cfg, f) for f in FIELDS), mb + 1, 0)
        assert L.tld_train_create(C.byref(c), C.byref(h)) == TLD_ERR_INVALID, vars(cfg)
        assert h.value is None and words.encode() in L.tld_last_error(), L.tld_last_error()


# ---- the CLIP towers ---------------------------------------------------------------------------------------------------------------------------------------------
# (rows per sample, width, patches, padded patch length) -> the largest max_batch: f [T, 4 W] bf16 below 4 GiB, the patch matrix, one sample per block of the y axis
CLIP = [((77, 768, 0, 0), 9078, "the MLP activation"), ((257, 1024, 256, 640), 2040, "the MLP activation"), ((128, 1024, 0, 0), 4095, "the MLP activation"),
        ((5, 64, 4, 3072), 65535, "the attention kernel puts one sample on each block of the grid's y axis"), ((50, 64, 49, 3072), 14266, "the patch matrix")]


def test_clip_create_boundary(driver):
    for (rows, W, pr, pk), mb, _ in CLIP:
        assert mb == min((GIB4 - 1) // (rows * 4 * W * 2), (GIB4 - 1) // (pr * pk * 2) if pr else 10 ** 9, 65535)
    outs = driver([f"clip {mb + k} {rows} {W} {pr} {pk}" for (rows, W, pr, pk), mb, _ in CLIP for k in (0, 1)])
    for k, (_, mb, words) in enumerate(CLIP):
        assert outs[2 * k]["refusal"] == ""
        bad = outs[2 * k + 1]["refusal"]
        assert bad.startswith(f"max_batch={mb + 1}: ") and words in bad and f"the largest max_batch that fits is {mb};" in bad, bad


def test_clip_create_refuses_through_the_library_before_any_hip_call():
    L = _lib.lib()
    h = C.c_void_p()
    text = _lib.TldClipConfig(vocab_size=49408, context_length=77, width=768, heads=12, layers=12, embed_dim=768, max_batch=9079, device_id=0)
    assert L.tld_clip_create(C.byref(text), C.byref(h)) == TLD_ERR_INVALID and h.value is None
    assert b"the MLP activation" in L.tld_last_error() and b"the largest max_batch that fits is 9078;" in L.tld_last_error(), L.tld_last_error()
    vis = _lib.TldClipVisConfig(image_size=224, patch_size=14, width=1024, heads=16, layers=24, embed_dim=768, max_batch=2041, device_id=0)
    assert L.tld_clip_vis_create(C.byref(vis), C.byref(h)) == TLD_ERR_INVALID and h.value is None
    assert b"the MLP activation" in L.tld_last_error() and b"the largest max_batch that fits is 2040;" in L.tld_last_error(), L.tld_last_error()
    vis = _lib.TldClipVisConfig(image_size=224, patch_size=32, width=64, heads=1, layers=1, embed_dim=64, max_batch=14267, device_id=0)
    assert L.tld_clip_vis_create(C.byref(vis), C.byref(h)) == TLD_ERR_INVALID and b"the patch matrix" in L.tld_last_error(), L.tld_last_error()


# ---- the raw-buffer hooks ------------------------------------------------------------------------------------------------------------------------------------------
# (query, "" or words of the refusal).  Accepted rows are the sizes tests/test_gpu_large_offsets.py runs, and sizes past 4 GiB at the kernels that address in 64 bits.
HOOKS = [
    ("dwconv 2730 16 3072", ""), ("dwconv 5000 16 3072", ""),                   # the whole-image kernel: 64-bit addresses, 4.0 and 7.3 GiB
    ("dwconv 682 32 3072", ""), ("dwconv 683 32 3072", "the row-streaming kernel (grids that are multiples of 32) writes through 32-bit byte offsets"),
    ("dwconv 683 32 3072", "the largest batch that fits is 682"), ("dwconv 170 64 3072", ""), ("dwconv 171 64 3072", "the largest batch that fits is 170"),
    ("dwconv 1000 48 3072", ""),                                                  # the tiled kernel: 64-bit addresses (13 GiB)
    ("dwconv 6000000 48 3072", "workgroups"),
    ("attn_fwd 5461 256 12", ""), ("attn_fwd 65535 256 12", ""), ("attn_fwd 65536 256 12", "the grid's y and z axes (at most 65535 each)"),
    ("attn_fwd 65536 16 1", "the grid's y and z axes"), ("attn_fwd 70000 1024 12", ""), ("attn_fwd 60000000 1024 12", "32-bit workgroup count"),
    ("attn_bwd 3640 256 12", ""), ("attn_bwd 100000 1024 12", ""), ("attn_bwd 6000000 1024 12", "32-bit workgroup count"),
    ("wgrad 524288 3072 768", ""), ("wgrad 100000000 3072 768", ""), ("wgrad 64 8388608 256", "below 2^24 bytes"), ("wgrad 64 256 8388608", "below 2^24 bytes"),
    ("gemm 699051 768 3072 3072 3072 0 0 0", ""), ("gemm 699052 768 3072 3072 3072 0 0 0", "beyond the 4 GiB reach of the 32-bit DMA offsets"),
    ("gemm 16777216 64 64 64 64 0 0 0", ""), ("gemm 16777217 64 64 64 64 0 0 0", "beyond the 4 GiB reach"),
    ("gemm 1398100 768 3072 3072 3072 1 0 0", ""), ("gemm 1398104 768 3072 3072 3072 1 0 0", "beyond the 4 GiB reach"),
    ("gemm 256 256 8388608 8388608 8388608 0 0 0", "beyond the 4 GiB reach"),    # a row pitch of 2^24 bytes
]


def test_hook_refusals(driver):
    outs = driver([q for q, _ in HOOKS])
    for (q, words), o in zip(HOOKS, outs):
        assert (o["refusal"] == "") if not words else (words in o["refusal"]), (q, o)


def test_hooks_refuse_through_the_library_before_any_hip_call():
    """Non-null pointers that are never dereferenced: each hook answers TLD_ERR_INVALID with its reason before it asks which device a pointer is on."""
    L = _lib.lib()
    buf = (C.c_float * 16)()
    p = C.c_void_p((C.addressof(buf) + 15) & ~15)              # (the GEMM hook checks its operands' alignment first)
    fp = C.cast(p, C.POINTER(C.c_float))

    def refused(rc, words):
        assert rc == TLD_ERR_INVALID and words in L.tld_last_error(), (rc, L.tld_last_error())

    refused(L.tld_debug_dwconv_gelu(p, fp, fp, p, 683, 32, 3072, None), b"the largest batch that fits is 682")
    refused(L.tld_debug_dwconv_gelu(p, fp, fp, p, 171, 64, 3072, None), b"32-bit byte offsets")
    refused(L.tld_debug_attention_fwd(p, p, p, 65536, 256, 12, 1, None, None), b"y and z axes")
    refused(L.tld_debug_attention_bwd(p, p, p, p, p, p, 6000000, 1024, 12, None), b"32-bit workgroup count")
    refused(L.tld_debug_wgrad(p, p, p, p, 1 << 20, 64, 1 << 23, 256, None), b"below 2^24 bytes")
    a = _lib.TldGemmEpilogueArgs()
    a.A = a.W = a.c_f32 = p
    a.M, a.N, a.K, a.lda, a.ldw, a.ldc, a.epilogue = 699052, 768, 3072, 3072, 3072, 768, 0
    refused(L.tld_debug_gemm_epilogue(C.byref(a), None), b"beyond the 4 GiB reach of the 32-bit DMA offsets")

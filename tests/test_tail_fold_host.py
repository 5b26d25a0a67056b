"""Host: the folded out_proj operand (csrc/tld_tail_fold_math.h) against a numpy float64 restatement, bit for bit.

W'[f][j] = float(sum_k double(Wout[f][k]) * double(bf16(Wd[k][j]))), b'[f] = float(sum_k double(Wout[f][k]) * double(bd[k]) + double(bo[f])), the sums
k-ascending with one add per element; the split bf16 image [2][pdp][d + hid] of [Wout | W'].  tests/host/tail_fold_main.cpp is compiled on its own
(the header has no HIP in it) and run on three shapes; the same program runs once under -fsanitize=address,undefined.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from weight_image_refs import _bf16_value, _reference      # (the restatement lives with those of the other weight images)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(16, 768, 3072), (4, 64, 128), (64, 192, 384)]      # (patch_dim, d, hid): the 100M model, the smallest, the widest patch


def _cxx():
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    return cxx


def _build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.run([_cxx(), "-std=c++17", *flags, "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc"),
                    os.path.join(REPO, "tests", "host", "tail_fold_main.cpp"), "-o", exe], check=True)
    return exe


def _inputs(pd, d, hid, seed):
    rng = np.random.default_rng(seed)
    wout = (rng.standard_normal((pd, d)) / np.sqrt(d)).astype(np.float32)
    wd = (rng.standard_normal((d, hid)) / np.sqrt(hid)).astype(np.float32)
    bd = (rng.standard_normal(d) * 0.1).astype(np.float32)
    bo = (rng.standard_normal(pd) * 0.1).astype(np.float32)
    return wout, wd, bd, bo


def _run(exe, tmp_path, pd, d, hid, seed):
    wout, wd, bd, bo = _inputs(pd, d, hid, seed)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        for a in (wout, wd, bd, bo):
            f.write(a.tobytes())
    r = subprocess.run([exe, str(pd), str(d), str(hid), fin, fout], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    raw = open(fout, "rb").read()
    pdp, K = (pd + 15) // 16 * 16, d + hid
    wf = np.frombuffer(raw, np.float32, pd * hid).reshape(pd, hid)
    bf = np.frombuffer(raw, np.float32, pd, offset=4 * pd * hid)
    img = np.frombuffer(raw, np.uint16, 2 * pdp * K, offset=4 * (pd * hid + pd)).reshape(2, pdp, K)
    return (wout, wd, bd, bo), (wf, bf, img)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tail_fold"), "tail_fold_main", ["-O2"])


@pytest.mark.parametrize("pd,d,hid", SHAPES)
def test_folded_operand_equals_the_float64_restatement(exe, tmp_path, pd, d, hid):
    ins, (wf, bf, img) = _run(exe, tmp_path, pd, d, hid, seed=pd + d)
    rwf, rbf, rimg = _reference(*ins)
    assert np.array_equal(wf.view(np.uint32), rwf.view(np.uint32)), f"W': {(wf != rwf).sum()} of {wf.size} elements differ"
    assert np.array_equal(bf.view(np.uint32), rbf.view(np.uint32)), "b' differs"
    assert np.array_equal(img, rimg), "split bf16 image differs"
    # the split keeps 16 significant bits of every weight: hi + lo is within 2^-16 of it, relative (a numerical statement of what the image is for)
    row = np.concatenate([ins[0], rwf], axis=1).astype(np.float64)
    rec = _bf16_value(img[0, :pd]).astype(np.float64) + _bf16_value(img[1, :pd]).astype(np.float64)
    assert np.all(np.abs(rec - row) <= 2.0 ** -16 * np.abs(row) + 1e-38)


def test_driver_is_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The stand-alone program (its own main, nothing loaded into Python) under -fsanitize=address,undefined, on the smallest shape and the widest patch."""
    san = _build(tmp_path, "tail_fold_main_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    for pd, d, hid in SHAPES[1:]:
        ins, (wf, bf, img) = _run(san, tmp_path, pd, d, hid, seed=3)
        rwf, rbf, rimg = _reference(*ins)
        assert np.array_equal(wf.view(np.uint32), rwf.view(np.uint32)) and np.array_equal(bf.view(np.uint32), rbf.view(np.uint32)) and np.array_equal(img, rimg)

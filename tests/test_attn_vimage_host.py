"""CPU: the row-major LDS image of V of the fused QKV + attention epilogues (csrc/tld_attn_vimage.h) -- its write map, the lane addresses of the
transposing read and the LDS map of the two-head epilogue -- through tests/host/attn_vimage_main.cpp, built plain and under AddressSanitizer + UBSan and run
directly.  The kernels include the same header, so these are the functions that run on the device.

The driver fills an image through the write map (both column maps: 32 features per wave column in the one-head form, 16 in the pair form) with the code
key * 64 + feature, emulates ds_read_b64_tr_b16 from its lane map (per 16 lanes: lane 4q + p supplies row q, columns 4p .. 4p + 3; lane i receives column i,
row q in element q) and checks, for all 64 lanes x 16 steps x 2 feature tiles x 2 reads: the values (feature 32 ct + l31, keys 16 s2 + 8 rd + 4 hi + 0 .. 3 in
order), 8-byte alignment, 64 distinct banks per 32-lane half under (addr / 4) % 64, and for every wave-level 8-byte write at most 4 lanes per bank under
(addr / 4) % 32 -- the floor for 512 bytes through 32 banks, and what the K / Q writes have."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mains(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler is needed (the oracle's Makefile needs one too)"
    out = tmp_path_factory.mktemp("attn_vimage")
    src = [os.path.join(REPO, "tests", "host", "attn_vimage_main.cpp"), "-I", os.path.join(REPO, "transformer_latent_diffusion_amd", "csrc")]
    exes = []
    for tag, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(out / f"attn_vimage_main_{tag}")
        subprocess.run([cxx, "-std=c++17", *flags, *src, "-o", exe], check=True)
        exes.append(exe)
    return exes


def _run(exe, *args):
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, (exe, args, r.stdout[-3000:], r.stderr[-2000:])
    return r.stdout


def test_image_values_alignment_and_banks(mains):
    for exe in mains:
        out = _run(exe, "check")
        assert out.split() == ["OK", str(2 * 64 * 16 * 2 * 2), "reads"], out          # both column maps x lanes x steps x feature tiles x reads


def test_pair_lds_map_phases_are_disjoint_and_inside_the_cu(mains):
    for exe in mains:
        rows = [ln.split() for ln in _run(exe, "map").splitlines()]
        phases = {ph: [(n, int(b), int(e)) for p2, n, b, e in rows if p2 == ph] for ph in ("1", "2")}
        assert [n for n, _, _ in phases["1"]] == ["tables", "K_A", "V_A", "Q", "K_B"] and [n for n, _, _ in phases["2"]] == ["V_B", "K_A", "V_A", "Q", "K_B"]
        for regs in phases.values():
            for k, (n, b, e) in enumerate(regs):
                assert 0 <= b < e <= 163840, (n, b, e)
                assert n == "tables" or e - b == 32768, (n, b, e)
                for n2, b2, e2 in regs[k + 1:]:
                    assert e <= b2 or e2 <= b, (n, n2)
        assert sum(e - b for _, b, e in phases["2"]) == 163840          # five images: the CU's 160 KiB, to the byte
        assert dict((n, (b, e)) for n, b, e in phases["1"])["tables"] == (0, 256 * 64 + 256 * 8 + 2 * 384 * 4)

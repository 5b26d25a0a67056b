"""GPU: the fused QKV + attention kernels reproduce, bit for bit, what the build BEFORE the row-major V image and the LDS-resident second head left behind
(DESIGN.md 4.2, 4.6).  tests/golden/qkv_attn_parent_bits.json holds the SHA-256 of `blk0.att`, `blk1.att` and the forward output (the latents, for the sampler)
recorded from that build by tools/record_attn_bits.py; the engine is bit-reproducible across boxes.  Every value written to LDS is the same bf16
and every MFMA gets the same operand elements in the same k-slots, so nothing may move.

Cases, all at d = 768, n_layers = 2, 256 tokens (the smallest width that reaches the fused kernel): batch 2 (12 head pairs); batch 45 (270 pairs: on 256 CUs
some workgroups run a second tile -- the images overlay what the next K-step and the tables land in, and the slot is used again); batch 45 again in the same
process; the 4-step CFG sampler on 2 images (block 0 on the shared half batch).  Each under TLD_QKV_ATTN_PAIR = 0 (one-head tiles, launch-path bit 11) and
= 2 (two-head tiles, bit 61), one subprocess per value running tools/record_attn_bits.py --mode."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_BIT, ONE_HEAD_BIT = 61, 11
CASES = ("b2", "b45", "b45_again", "cfg")

with open(os.path.join(REPO, "tests", "golden", "qkv_attn_parent_bits.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def runs():
    spec = importlib.util.spec_from_file_location("record_attn_bits", os.path.join(REPO, "tools", "record_attn_bits.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    return {mode: rec.run_mode(mode) for mode in (0, 2)}


def test_golden_covers_the_cases_and_the_recorded_paths_are_the_intended_kernels():
    for mode, want, other in ((0, ONE_HEAD_BIT, PAIR_BIT), (2, PAIR_BIT, ONE_HEAD_BIT)):
        assert sorted(GOLDEN[str(mode)]) == sorted(CASES)
        for case in CASES:
            paths = GOLDEN[str(mode)][case]["paths"]
            assert (paths >> want) & 1 and not (paths >> other) & 1, (mode, case, hex(paths))
    for case in CASES:          # the parent's two forms agree with each other (tests/test_gpu_qkv_pair.py), so do their records
        assert GOLDEN["0"][case]["sha256"] == GOLDEN["2"][case]["sha256"], case


@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("case", CASES)
def test_bits_of_the_parent_build(runs, mode, case):
    got, want = runs[mode][case], GOLDEN[str(mode)][case]
    bit, other = (PAIR_BIT, ONE_HEAD_BIT) if mode == 2 else (ONE_HEAD_BIT, PAIR_BIT)
    assert (got["paths"] >> bit) & 1 and not (got["paths"] >> other) & 1, (mode, case, hex(got["paths"]))         # the intended kernel ran
    print(mode, case, got["sha256"])
    assert got["sha256"] == want["sha256"], (mode, case)

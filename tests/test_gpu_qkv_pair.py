"""GPU: the fused QKV + attention kernel on two-head tiles (EPI_QKV_ATTN2) against its one-head form.  Both give every output element the
same K order, the same LayerNorm correction, the same rounding of q, k, v to bf16 and the same attention arithmetic, so `blkN.att` and the forward output must be
BITWISE equal.  TLD_QKV_ATTN_PAIR is read when an engine is created: one subprocess per value (0 never, 2 wherever the shape permits, 1 by the rule), each
running every case once; the tests compare what they left.

Cases (a), (c) and (d) are at d = 384, where the engine does not fold LayerNorm-1 (3 d is no multiple of 256) and so runs the two-kernel path under every value
of the switch: there the comparison holds that the switch changes nothing.  Cases (b), (e) and (f) -- d = 768, the width of the benchmarked model -- are the ones
that run the two kernels against each other, and they assert it from the recorded launch paths: (e) and (f) repeat what (c) and (d) are about (a second tile per
workgroup, the sampler's shared half batch) at a width that takes the fused kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIR_BIT, ONE_HEAD_BIT = 61, 11

SCRIPT = r"""
import sys, numpy as np, torch
sys.path.insert(0, REPO)
from dataclasses import asdict
from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator, _lib
from transformer_latent_diffusion_amd.weights import synth_state_dict
mode, out_path = int(sys.argv[1]), sys.argv[2]
dev = torch.device("cuda:0")
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

def model(d, seed):
    cfg = DenoiserConfig(image_size=32, n_channels=4, embed_dim=d, n_layers=2)
    m = Denoiser(**asdict(cfg)).to(dev)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, seed).items()})
    return m

def inputs(batch, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((batch, 4, 32, 32)).astype(np.float32), rng.uniform(0.02, 0.98, (batch, 1)).astype(np.float32),
            (rng.standard_normal((batch, 768)) * 0.5).astype(np.float32))

def forward(m, batch, seed, res, tag):
    x, s, lab = inputs(batch, seed)
    m.reserve(batch); m.set_debug(True)
    res[tag + ".out"] = m(t(x), t(s), t(lab)).float().cpu().numpy()
    res[tag + ".paths"] = np.array([m.debug_paths()], dtype=np.uint64)
    for l in (0, 1):
        res[f"{tag}.att{l}"] = m.read_stage(f"blk{l}.att")

res = {}
if mode in (0, 2):
    m384, m768 = model(384, 5), model(768, 6)
    forward(m384, 3, 11, res, "a")           # 9 head pairs: fewer than CUs, 6 K-steps
    forward(m768, 2, 12, res, "b")           # 12 K-steps, 6 pairs per sample
    forward(m384, 90, 13, res, "c")          # 270 pairs: on 256 CUs some workgroups run a second tile (slot reuse, cold restart after an epilogue)
    forward(m384, 90, 13, res, "c2")         # ... and once more in the same process
    forward(m768, 45, 16, res, "e")          # the same 270 pairs at the width that takes the fused kernel: a second tile, the slot and the LDS images used again
    forward(m768, 45, 16, res, "e2")
    x, s, lab = inputs(2, 14)                # the sampler with CFG: block 0 runs on the shared half batch
    gen = DiffusionGenerator(m384, None, dev, torch.float32)
    res["d.lat"] = gen.generate_latents(torch.from_numpy(lab), n_iter=4, num_imgs=2, class_guidance=3.0, seeds=torch.from_numpy(x), img_size=32,
                                        sharp_f=0.0, bright_f=0.0).float().cpu().numpy()
    gen = DiffusionGenerator(m768, None, dev, torch.float32)
    res["f.lat"] = gen.generate_latents(torch.from_numpy(lab), n_iter=4, num_imgs=2, class_guidance=3.0, seeds=torch.from_numpy(x), img_size=32,
                                        sharp_f=0.0, bright_f=0.0).float().cpu().numpy()
else:
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    full = next(b for b in range(1, 4096) if (b * 6) % cus == 0)          # d = 768: 12 heads = 6 pairs per sample; whole rounds of pairs
    q = np.array([full, 12, cus, 2, 12, cus], dtype=np.int32); plan = np.zeros(2, dtype=np.int32)
    _lib.check(_lib.lib().tld_debug_qkv_pair_plan(q.ctypes.data, 2, plan.ctypes.data, None), "plan")
    res["rule.plan"] = plan; res["rule.batch"] = np.array([full])
    forward(model(768, 6), full, 15, res, "rule_full")
    forward(model(768, 6), 2, 12, res, "rule_small")
np.savez(out_path, **res)
print("DONE")
""".replace("REPO", repr(REPO))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("qkv_pair")
    script = d / "run.py"
    script.write_text(SCRIPT)
    out = {}
    for mode in (0, 2, 1):
        path = str(d / f"mode{mode}.npz")
        r = subprocess.run([sys.executable, str(script), str(mode), path], capture_output=True, text=True, env=dict(os.environ, TLD_QKV_ATTN_PAIR=str(mode)),
                           timeout=600)
        assert r.returncode == 0 and "DONE" in r.stdout, (mode, r.stdout[-1500:], r.stderr[-3000:])
        out[mode] = dict(np.load(path))
    return out


def _bit(paths, bit):
    return bool((int(paths[0]) >> bit) & 1)


@pytest.mark.parametrize("case", ["a", "b", "c", "e"])
def test_two_head_tiles_give_the_bits_of_one_head_tiles(runs, case):
    one, two = runs[0], runs[2]
    fused = _bit(one[case + ".paths"], ONE_HEAD_BIT)          # this width runs the fused kernel at all
    assert fused or case in "ac", case                        # (b) and (e) must: the comparison is between the two kernels ...
    assert not _bit(one[case + ".paths"], PAIR_BIT)
    assert _bit(two[case + ".paths"], PAIR_BIT) == fused and not _bit(two[case + ".paths"], ONE_HEAD_BIT)
    for k in (".att0", ".att1", ".out"):
        a, b = one[case + k], two[case + k]
        assert np.isfinite(a).all() and a.shape == b.shape and np.abs(a).max() > 0
        assert np.array_equal(a, b), (case + k, int((a != b).sum()), a.size)                          # ... and bitwise


def test_second_run_in_one_process_gives_the_same_bits(runs):
    """Cases (c) and (e) again in the same process: the park / reload of the second head and the LDS overlays leave no trace of the run before."""
    for mode in (0, 2):
        for case in "ce":
            for k in (".att0", ".att1", ".out"):
                assert np.array_equal(runs[mode][case + k], runs[mode][case + "2" + k]), (mode, case, k)


def test_sampler_with_cfg_gives_the_same_latents(runs):
    for case in "df":
        a, b = runs[0][case + ".lat"], runs[2][case + ".lat"]
        assert np.isfinite(a).all() and np.array_equal(a, b), (case, int((a != b).sum()))


def test_rule_takes_pairs_for_whole_rounds_and_one_head_tiles_for_batch_2(runs):
    r = runs[1]
    assert list(r["rule.plan"]) == [1, 0], (r["rule.plan"], r["rule.batch"])
    assert _bit(r["rule_full.paths"], PAIR_BIT), r["rule.batch"]
    assert _bit(r["rule_small.paths"], ONE_HEAD_BIT) and not _bit(r["rule_small.paths"], PAIR_BIT)
    for k in (".att0", ".att1", ".out"):                         # batch 2 under the rule is case (b) of the one-head arm: the same engine mode, the same bits
        assert np.array_equal(r["rule_small" + k], runs[0]["b" + k]), k

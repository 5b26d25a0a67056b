#!/usr/bin/env python3
"""SHA-256 of what the fused QKV + attention kernels leave behind -- `blk0.att`, `blk1.att` and the forward output (the latents, for the sampler case) -- at
d = 768, n_layers = 2, 256 tokens, under TLD_QKV_ATTN_PAIR = 0 (one-head tiles) and = 2 (two-head tiles wherever the shape permits).

    python tools/record_attn_bits.py --mode 0          one engine mode in this process: prints one JSON line {case: {"paths": int, "sha256": {...}}}
    python tools/record_attn_bits.py --out FILE.json   both modes, one subprocess each: writes {"0": {...}, "2": {...}}

tests/golden/qkv_attn_parent_bits.json was written by the second form from the build BEFORE the V image became row-major; the engine is
bit-reproducible across boxes, and tests/test_gpu_attn_vimage.py holds every later build to those hashes through the first form.

Cases: b2 = batch 2 (12 head pairs); b45 = batch 45 (270 pairs: on 256 CUs some workgroups run a second tile, so the images overlay what the next K-step and
tables land in, and the slot is used again); b45_again = the same in the same process; cfg = the 4-step CFG sampler on 2 images (block 0 on the shared half batch)."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (0, 2)


def sha(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    return hashlib.sha256(str((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def worker():
    import numpy as np
    import torch
    sys.path.insert(0, REPO)
    from dataclasses import asdict
    from transformer_latent_diffusion_amd import Denoiser, DenoiserConfig, DiffusionGenerator
    from transformer_latent_diffusion_amd.weights import synth_state_dict

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cfg = DenoiserConfig(image_size=32, n_channels=4, embed_dim=768, n_layers=2)
    m = Denoiser(**asdict(cfg)).to(dev)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 6).items()})

    def inputs(batch, seed):
        rng = np.random.default_rng(seed)
        return (rng.standard_normal((batch, 4, 32, 32)).astype(np.float32), rng.uniform(0.02, 0.98, (batch, 1)).astype(np.float32),
                (rng.standard_normal((batch, 768)) * 0.5).astype(np.float32))

    res = {}

    def stages(tag, out):
        res[tag] = {"paths": int(m.debug_paths()),
                    "sha256": {"att0": sha(m.read_stage("blk0.att")), "att1": sha(m.read_stage("blk1.att")), "out": sha(out)}}

    def forward(batch, seed, tag):
        x, s, lab = inputs(batch, seed)
        m.reserve(batch); m.set_debug(True)
        stages(tag, m(t(x), t(s), t(lab)).float().cpu().numpy())

    forward(2, 12, "b2")
    forward(45, 16, "b45")
    forward(45, 16, "b45_again")
    x, _, lab = inputs(2, 14)
    m.set_debug(True)
    gen = DiffusionGenerator(m, None, dev, torch.float32)
    lat = gen.generate_latents(torch.from_numpy(lab), n_iter=4, num_imgs=2, class_guidance=3.0, seeds=torch.from_numpy(x), img_size=32, sharp_f=0.0, bright_f=0.0)
    stages("cfg", lat.float().cpu().numpy())
    print("BITS " + json.dumps(res, sort_keys=True), flush=True)


def run_mode(mode, timeout=600):
    """The cases under TLD_QKV_ATTN_PAIR = mode in a fresh process (the switch is read when an engine is created)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--mode", str(mode)], capture_output=True, text=True,
                       env=dict(os.environ, TLD_QKV_ATTN_PAIR=str(mode)), timeout=timeout)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("BITS ")), None)
    if r.returncode or line is None:
        raise RuntimeError(f"mode {mode}: rc {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}")
    return json.loads(line[5:])


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", type=int, choices=MODES)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode is not None:
        worker()
    else:
        rec = {str(mode): run_mode(mode) for mode in MODES}
        text = json.dumps(rec, indent=1, sort_keys=True) + "\n"
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(text)
        print(text, end="")

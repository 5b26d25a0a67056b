#!/usr/bin/env python3
"""Dump the g5 forward, a 70-sample forward, the g5 35-step CFG end latent and the tiny model's sampler outputs (end latent and both traces of a plain call, a
strength-0.65 call, a masked call and the five-request call of tests/test_gpu_requests.py) of the engine library selected by TLD_LIB (same-box A/B of builds:
outputs of two builds that only re-order work must be BITWISE equal).  One "part <name> <sha1>" line per tensor: equal lines are equal bits.
Then the VAE: a tiny decoder (latent side 8: one sample per attention step, no fused GroupNorm statistics; side 16: batched attention, fused statistics)
and a tiny encoder (64 px, fp32 and bf16 input), B = 2 -- the output and every captured stage as parts, plus a "vae <name> weight_bytes ... launches ..." line each.
Then the CLIP text tower with the stage hook off: encode_text of the cases of tests/test_gpu_clip.py (tiny chunked, ViT-L/14 at 4 prompts, both g13 geometries)
and of 64 prompts on a two-layer ViT-L/14 tower; and the CLIP image tower: a 5-token tower chunked (5 images, 2 per call; fp32 and bf16 pixels) and a 257-token case.
Then the stage hooks ON: one forward of the tiny denoiser, one encode of the tiny text tower and of the tiny image tower and one tiny training step (loss, gradient vector), each with
every stage its header block names as a part ("absent <name>" where the engine's path has no such stage).
Then three more training steps with the hook off (loss and gradient vector): d 256, image 64, one block, batch 5 with the untransposed and, under TLD_TRAIN_TN_WGRAD=0, the
transposing weight-gradient split; d 192, image 24, two blocks, batch 3: the zero-padded form.
Then five forwards with the hook off, the smallest shapes that reach the row and attention launch forms (csrc/tld_launch_plan.h) the cases above do not: d 192 at 12 x 12
tokens (plain embed, generic LayerNorm, masked attention, the VALU cross_row, whole-image depthwise); d 256 at 20 x 20 (four-features-per-lane LayerNorm, the tiled depthwise);
d 256 at 32 x 32 under TLD_FUSE_DWCONV=0 (chunked attention, streaming depthwise); the same 20 x 20 model with fp8 operands (quantising LayerNorm, cross_row and depthwise, the
unfolded matrix-pipe tail); d 384 at 8 x 8 in low-latency class 1 (one-chunk attention at 64 tokens, the split-K finish).
    TLD_LIB=<lib.so> python tools/lib_ab_check.py out.npy"""
import hashlib, os, sys
from dataclasses import asdict
import numpy as np, torch
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, R); sys.path.insert(0, os.path.join(R, "tests"))
from conftest import cfg_from_arr, load_golden, rel_rms, synth_weights
from transformer_latent_diffusion_amd import Denoiser
g = load_golden("g5_100m.npz")
cfg = cfg_from_arr(g["cfg"]); sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
dev = torch.device("cuda:0")
m = Denoiser(**asdict(cfg)).to(dev); m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
out = m(t(g["x"]), t(g["sigma"]), t(g["label"])).cpu().numpy()
rng = np.random.default_rng(3)
x = rng.standard_normal((70, 4, 32, 32)).astype(np.float32); s = rng.uniform(0.02, 0.98, (70, 1)).astype(np.float32)
lab = (rng.standard_normal((70, 768)) * 0.5).astype(np.float32)
big = m(t(x), t(s), t(lab)).cpu().numpy()
print(os.path.basename(os.environ.get("TLD_LIB", "default")), "g5 forward rel-rms", rel_rms(out, g["x0"]), "finite", bool(np.isfinite(big).all()))
from transformer_latent_diffusion_amd import DiffusionGenerator
lat = DiffusionGenerator(m, None, dev, torch.float32).generate_latents(torch.from_numpy(g["traj_labels"]), n_iter=int(g["traj_n_iter"]), num_imgs=1,
                                                                       class_guidance=float(g["traj_class_guidance"]), seeds=torch.from_numpy(g["traj_seeds"]),
                                                                       img_size=32, sharp_f=0.0, bright_f=0.0).cpu().numpy()
print("g5 35-step end latent rel-rms", rel_rms(lat, g["traj_latent"]))
parts = {"g5 forward": out, "70-sample forward": big, "g5 35-step end latent": lat}
# the sampler entries on the tiny model (inputs, mask and requests as tests/test_gpu_requests.py builds them)
gt = load_golden("g2_tiny32_sampler.npz")
ct = cfg_from_arr(gt["cfg"]); sdt = synth_weights(ct, gt["weight_seed"], gt["weight_checksum"])
mt = Denoiser(**asdict(ct)).to(dev); mt.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sdt.items()})
gent = DiffusionGenerator(mt, None, dev, torch.float32)
rg = torch.Generator().manual_seed(61)
eps = torch.randn(5, 4, 32, 32, generator=rg); z0 = torch.randn(5, 4, 32, 32, generator=rg) * 0.5; labels = torch.randn(5, 768, generator=rg) * 0.5
mask = torch.zeros(5, 1, 32, 32); mask[:, :, 5:21, 3:17] = 1
kw = dict(n_iter=8, class_guidance=3.0, sharp_f=0.1, bright_f=0.1, seeds=eps, trace=True)
five = dict(class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], n_iter=[8, 5, 8, 3, 5], use_ddpm_plus=[True, True, False, True, True], exponent=[1, 1, 1, 1, 2])
calls = {"tiny plain": lambda: gent.generate_latents(labels, num_imgs=5, img_size=32, **kw),
         "tiny strength 0.65": lambda: gent.generate_latents_from(z0, labels, strength=0.65, **kw),
         "tiny masked": lambda: gent.generate_latents_from(z0, labels, strength=0.65, mask=mask, **kw),
         "tiny five requests": lambda: gent.generate_latents_requests(labels, seeds=eps, img_size=32, sharp_f=0.1, bright_f=0.1, trace=True, **five)}
for name, call in calls.items():
    for what, v in zip(("end latent", "trace_x0", "trace_xt"), call()):
        parts[f"{name} {what}"] = v.cpu().numpy()
# the VAE engines: (64, 128), one layer per block, B = 2 -- the smallest shapes that reach every host path the two engines share
import warnings
from transformer_latent_diffusion_amd.vae import AutoencoderKLDecoder, VaeDecoderConfig
from transformer_latent_diffusion_amd.vae_encoder import AutoencoderKLEncoder, VaeEncoderConfig
warnings.simplefilter("ignore", RuntimeWarning)            # (the synthetic-weights notice)
mid = ["mid.res0", "mid.attn", "mid.res1"]
dec_stages = ["conv_in"] + mid + ["up0.res0", "up0.res1", "up0.upsample", "up1.res0", "up1.res1", "norm_out"]
enc_stages = ["conv_in", "down0.res0", "down0.downsample", "down1.res0"] + mid + ["norm_out"]
def vae_parts(name, eng, call, inp, stages):
    call(inp)                                               # builds the engine
    eng.set_debug(True); eng.set_profile(True)
    parts[name] = call(inp).cpu().numpy()
    for st in stages:
        parts[f"{name} {st}"] = eng.read_stage(st).numpy()
    print("vae", name, "weight_bytes", eng.weight_bytes, "launches", {k: n for k, (_, n) in eng.get_profile().items()})
dec = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=4, max_batch=2)
for side in (8, 16):
    vae_parts(f"vae decode {side}", dec, lambda z: dec.decode(z)[0], torch.randn(2, 4, side, side, generator=rg).to(dev), dec_stages)
enc = AutoencoderKLEncoder(VaeEncoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=4, max_batch=2)
img = (torch.randn(2, 3, 64, 64, generator=rg) * 0.6).clamp(-1, 1)
for dt in (torch.float32, torch.bfloat16):
    vae_parts(f"vae encode {dt}".replace("torch.", ""), enc, enc.moments, img.to(dt).to(dev), enc_stages)
# the CLIP text tower, debug off: the cases of tests/test_gpu_clip.py and the shipped batch of 64 prompts
from test_clip_host import TINY, _tokens, load_g13
from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder, synth_clip_state_dict
def clip_part(name, ccfg, csd, text, max_batch):
    ce = ClipTextEncoder(ccfg, max_batch=max_batch)
    ce.load_state_dict({k: torch.from_numpy(v) for k, v in csd.items()})
    parts[name] = ce.to(dev).encode_text(text.to(dev)).cpu().numpy()
    ce._drop_engine()
clip_part("clip tiny 11 prompts", TINY, synth_clip_state_dict(TINY, 3), _tokens(TINY, 11, 1), 4)
clip_part("clip l14 4 prompts", ClipTextConfig(), synth_clip_state_dict(ClipTextConfig(), 0), _tokens(ClipTextConfig(), 4, 2), 4)
for tag in ("tiny", "l14"):
    gcfg, gsd, gtext, _, _ = load_g13(tag)
    clip_part(f"clip g13 {tag}", gcfg, gsd, gtext, 8)
c2 = ClipTextConfig(layers=2)
clip_part("clip l14 two layers 64 prompts", c2, synth_clip_state_dict(c2, 0), _tokens(c2, 64, 5), 64)
# the CLIP image tower, debug off: the tiny tower chunked (5 images, 2 per call) in fp32 and bf16 pixels, and the 257-token case of tests/test_gpu_clip_vision.py
from test_clip_vision_host import CASES, case_pixels, case_weights, vcfg
from transformer_latent_diffusion_amd.clip_image import ClipImageEncoder, synth_clip_visual_state_dict
def clip_vis_part(name, vc, vsd, pix, max_batch):
    ve = ClipImageEncoder(vc, max_batch=max_batch)
    ve.load_state_dict(vsd)
    parts[name] = ve.to(dev).encode_image(pix.to(dev)).cpu().numpy()
    ve._drop_engine()
vtiny = vcfg(14, 2, 64)
vtiny_sd = {k: torch.from_numpy(v) for k, v in synth_clip_visual_state_dict(vtiny, 3).items()}
vpix = torch.randn(5, 3, 28, 28, generator=rg)
for dt in (torch.float32, torch.bfloat16):
    clip_vis_part(f"clip_vis tiny 5 images {dt}".replace("torch.", ""), vtiny, vtiny_sd, vpix.to(dt), 2)
clip_vis_part("clip_vis T257W128", CASES["T257W128"][0], case_weights("T257W128"), case_pixels("T257W128"), CASES["T257W128"][2])
# the stage hooks on: every stage name of include/tld_hip.h is tried, so a stage that appears or disappears shows as a changed line
staged = set()
def stage_parts(tag, names, read):
    for n in names:
        try:
            parts[f"{tag} {n}"] = np.asarray(read(n), np.float32)
            staged.add(f"{tag} {n}")                         # (a stage may hold the poison where its kernel stores nothing: no finiteness check)
        except RuntimeError:
            print("absent", tag, n)
mt.reserve(2); mt.set_debug(True)
parts["tiny debug forward"] = mt(eps[:2].to(dev), torch.tensor([[0.3], [0.8]]).to(dev), labels[:2].to(dev)).cpu().numpy()
blk = ("x_in ln1 xn1 qk vt att sa ca stats xn3 hid_pre hid splitk mlp wqkv wup wdown qkv_c1 qkv_b1 up_c1 up_b1").split()
stage_parts("tiny stage", ["tokens0", "out"] + [f"cond.{n}" for n in "sin h1 pre y kv wq bwq".split()] + [f"blk{i}.{n}" for i in range(ct.n_layers) for n in blk],
            mt.read_stage)
from weight_image_refs import BLOCK_IMAGES, GLOBAL_IMAGES      # the weight images in storage order
stage_parts("tiny stage", GLOBAL_IMAGES + [f"blk{i}.{n}" for i in range(ct.n_layers) for n in BLOCK_IMAGES], mt.read_stage)
mt.set_debug(False)
ce = ClipTextEncoder(TINY, max_batch=4)
ce.load_state_dict({k: torch.from_numpy(v) for k, v in synth_clip_state_dict(TINY, 3).items()})
ce.to(dev).set_debug(True)
parts["clip tiny debug encode"] = ce.encode_text(_tokens(TINY, 3, 1).to(dev)).cpu().numpy()
cblk = "h1 qkv att attn_out x1 h2 f_pre f mlp_out x2 in_w out_w fc_w proj_w".split()
stage_parts("clip stage", ["x0", "pooled", "out", "proj_t"] + [f"blk{i}.{n}" for i in range(TINY.layers) for n in cblk], lambda n: ce.read_stage(n).numpy())
ce._drop_engine()
ve = ClipImageEncoder(vtiny, max_batch=4)
ve.load_state_dict(vtiny_sd)
ve.to(dev).set_debug(True)
parts["clip_vis tiny debug encode"] = ve.encode_image(vpix[:3].to(dev)).cpu().numpy()
stage_parts("clip_vis stage", ["patches", "emb", "x0", "pooled", "out", "conv_w", "proj_t"] + [f"blk{i}.{n}" for i in range(vtiny.layers) for n in cblk],
            lambda n: ve.read_stage(n).numpy())
ve._drop_engine()
from transformer_latent_diffusion_amd import Trainer
tr = Trainer(ct, device=dev, state_dict={k: torch.from_numpy(np.array(v)) for k, v in sdt.items()}, max_batch=2).set_debug(True)
loss, pred = tr.forward_backward((0.6 * z0[:2] + 0.4 * eps[:2]).contiguous(), torch.tensor([0.4, 0.7]), labels[:2], z0[:2])
torch.cuda.synchronize()
parts["train loss"] = loss.float().cpu().numpy().reshape(-1); parts["train prediction"] = pred.float().cpu().numpy(); parts["train gradients"] = tr.grads.cpu().numpy()
tblk = ("x1 a1 qk vt att x2 a2 qc cr x3 a3 h hc o st1 st2 st3 p0 kvc wqkv wq wup wdown wqkv_t wq_t wup_t wdown_t gl gx.in dg dhc dh da3 gx.ln3 dqc dkv da2 gx.ln2 dqkv da1 "
        "gx.ln1 gxb.ln1").split()
stage_parts("train stage", "sinb h1 g1v ycat y yst p16 p16n est1 e est2 xfin dout row_loss gx.tail gxb.tail dy de dpn dp16 dycat dg1".split() +
            [f"blk{i}.{n}" for i in range(ct.n_layers) for n in tblk], lambda n: tr.read_stage(n).numpy())
tr.set_debug(False)
# three more training steps, stage hook off: the smallest shapes that reach each weight-gradient form (csrc/tld_train_plan.h) -- the untransposed split (sk 5 at
# 256 CUs), the transposing split (TLD_TRAIN_TN_WGRAD=0, read when the trainer is created) and the zero-padded form (M = 432)
from transformer_latent_diffusion_amd import DenoiserConfig
from transformer_latent_diffusion_amd.weights import synth_state_dict
def train_part(name, d, image, blocks, batch, tn_off=False):
    c = DenoiserConfig(image_size=image, noise_embed_dims=256, patch_size=2, embed_dim=d, dropout=0, n_layers=blocks, text_emb_size=768, n_channels=4, mlp_multiplier=4)
    old = os.environ.get("TLD_TRAIN_TN_WGRAD")
    if tn_off:
        os.environ["TLD_TRAIN_TN_WGRAD"] = "0"
    try:
        t2 = Trainer(c, device=dev, state_dict={k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(c, 31).items()}, max_batch=batch, keep_ema=False, use_graph=False)
    finally:
        if tn_off:
            os.environ.pop("TLD_TRAIN_TN_WGRAD") if old is None else os.environ.__setitem__("TLD_TRAIN_TN_WGRAD", old)
    gg = torch.Generator().manual_seed(32 + batch)
    x0 = torch.randn(batch, 4, image, image, generator=gg) * 0.8
    nz = torch.randn(batch, 4, image, image, generator=gg)
    lv = torch.rand(batch, generator=gg) * 0.9 + 0.05
    lb = torch.randn(batch, 768, generator=gg) * 0.5
    xn = (1 - lv).view(-1, 1, 1, 1) * x0 + lv.view(-1, 1, 1, 1) * nz
    ls, _ = t2.forward_backward(xn.contiguous(), lv, lb, x0)
    torch.cuda.synchronize()
    parts[f"{name} loss"] = ls.float().cpu().numpy().reshape(-1); parts[f"{name} gradients"] = t2.grads.cpu().numpy()
train_part("train d256 g32 untransposed split", 256, 64, 1, 5)
train_part("train d256 g32 transposing split", 256, 64, 1, 5, tn_off=True)
train_part("train d192 g12 zero-padded", 192, 24, 2, 3)
# forwards of the launch forms not reached above (csrc/tld_launch_plan.h), stage hook off
def forward_part(name, d, image, batch, env=None, setup=None):
    c = DenoiserConfig(image_size=image, noise_embed_dims=256, patch_size=2, embed_dim=d, dropout=0, n_layers=2, text_emb_size=768, n_channels=4, mlp_multiplier=4)
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        fm = Denoiser(**asdict(c)).to(dev)
        fm.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(c, 41).items()})
        if setup:
            setup(fm)
        gg = torch.Generator().manual_seed(43 + d + image)
        xs, sg, lb = torch.randn(batch, 4, image, image, generator=gg), torch.rand(batch, 1, generator=gg) * 0.9 + 0.05, torch.randn(batch, 768, generator=gg) * 0.5
        parts[name] = fm(xs.to(dev), sg.to(dev), lb.to(dev)).float().cpu().numpy()      # (the switches are read when the engine is created: at this first forward)
    finally:
        for k, v in old.items():
            os.environ.pop(k) if v is None else os.environ.__setitem__(k, v)
forward_part("forward d192 g12", 192, 24, 3)
forward_part("forward d256 g20", 256, 40, 3)
forward_part("forward d256 g32 unfused depthwise", 256, 64, 3, env={"TLD_FUSE_DWCONV": "0"})
forward_part("forward d256 g20 fp8", 256, 40, 3, setup=lambda fm: fm.set_gemm_dtype("fp8"))
forward_part("forward d384 g8 low latency", 384, 16, 2, setup=lambda fm: fm.set_low_latency(1))
for name, v in parts.items():
    assert name in staged or np.isfinite(v).all(), name
    print("part", name, tuple(v.shape), hashlib.sha1(np.ascontiguousarray(v).tobytes()).hexdigest())
np.save(sys.argv[1], np.concatenate([v.reshape(-1) for v in parts.values()]))

"""CPU: the call transcript of the Python sampler surface (denoiser.py, diffusion.py, sharded.py).

Every public entry is driven through a fixed list of calls around a stand-in for libtld_hip.so that records what ``tld_sample``,
``tld_sample_from`` and the four ``tld_sample_requests*`` entries receive: the entry, the batch, the level count and every scalar, each request record, which
optional pointers were null, and every tensor operand BY NAME -- a bitwise match against a table of tensors this file builds itself (the
``torch.randn`` draws from the same seeds, ``schedule.step_coefficients`` tables, stacked and filled optionals, ...), so the transcript holds
no hash of a random draw and does not depend on the torch or numpy build.  The stand-in reads its operands through host pointers and writes a
deterministic function of them into ``out`` and the trace slots the engine would write, so the un-sorting, dtype and decode code after the
call is recorded too: what each public call returned goes into the transcript as shapes, dtypes and names.  Refusals are recorded with the
exception type and the full message.  The transcript must equal tests/golden/sampler_surface_transcript.json, recorded with

    python tests/test_sampler_surface_host.py --record

at the commit before the three modules' copies were folded into one request-preparation path; only the public API is used."""
import contextlib
import ctypes as C
import json
import os
import sys
from dataclasses import asdict

import numpy as np
import torch
from torch import Tensor

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "sampler_surface_transcript.json")
S, CH, TXT = 16, 4, 768
IMG = (CH, S, S)
CPU = torch.device("cpu")


def _np(v):
    if isinstance(v, Tensor):
        v = v.detach().cpu().float().numpy()
    return np.ascontiguousarray(v, dtype=np.float32)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


class Names:
    """The table of expected tensors; ``of(v)`` names ``v`` by a bitwise match: a whole entry, one entry's rows gathered along axis 0 or 1
    (``name[[2, 0, 1]]``, ``name[:, [2, 0, 1]]``), one sub-tensor (``name[i]``), or a list of such names per row; ``?`` where nothing matches.
    A bfloat16 tensor is matched against the entries rounded to bfloat16."""

    def __init__(self):
        self.t, self.bf = [], {}

    def add(self, name, v):
        if all(n != name for n, _ in self.t):
            self.t.append((name, _np(v)))
        return v

    def _gather(self, t, a, axis):
        if t.ndim != a.ndim or a.ndim <= axis + 1 or t.shape[:axis] != a.shape[:axis] or t.shape[axis + 1:] != a.shape[axis + 1:]:
            return None
        tt, aa = np.moveaxis(t, axis, 0), np.moveaxis(a, axis, 0)
        perm = [next((i for i in range(len(tt)) if _same(np.ascontiguousarray(tt[i]), np.ascontiguousarray(row))), None) for row in aa]
        return None if None in perm else perm

    def of(self, v, rows=True):
        if v is None:
            return None
        bf = isinstance(v, Tensor) and v.dtype == torch.bfloat16
        a = _np(v)
        if a.size == 0:
            return f"empty{list(a.shape)}"
        for name, t in self.t:
            if bf:
                if name not in self.bf:
                    self.bf[name] = torch.from_numpy(t).to(torch.bfloat16).float().numpy()
                name, t = f"bf16({name})", self.bf[name]
            if _same(t, a):
                return name
            if t.ndim == a.ndim + 1 and t.shape[1:] == a.shape:
                for i in range(len(t)):
                    if _same(np.ascontiguousarray(t[i]), a):
                        return f"{name}[{i}]"
            for axis, pre in ((0, ""), (1, ":, ")):
                perm = self._gather(t, a, axis)
                if perm is not None:
                    return f"{name}[{pre}{perm}]"
        if rows and a.ndim > 1:
            return [self.of(v[k], rows=False) for k in range(len(a))]
        return "?"


class Lib:
    """Stands in for libtld_hip.so.  ``value`` of record k: 0.5 eps[k] + label[k, 0] + guidance + n_levels / 8 (+ start_mix / 4 x init[k])
    (+ mask[k]) (+ neg[k, 1] where the record has a negative label); prediction i of the trace is value + (i + 1), state i is value - (i + 1),
    written for i < n_levels - 1 only, as the engine leaves a finished request's slots alone."""

    def __init__(self, names, log, state):
        self.names, self.log, self.state = names, log, state

    @staticmethod
    def _arr(p, shape):
        a = p.value if isinstance(p, C.c_void_p) else p
        return None if a is None else np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_float)), shape=shape)

    def _run(self, entry, B, eps, lab, z0, m, neg, recs, coeffs, scalars, out, tx0, txt, stream):
        n = self.state["n"]
        self.state["n"] += 1
        e, l, z = self._arr(eps, (B,) + IMG), self._arr(lab, (B, TXT)), self._arr(z0, (B,) + IMG)
        mm, ng = self._arr(m, (B, 1, S, S)), self._arr(neg, (B, TXT))
        n_max = max(r[0] for r in recs)
        val = np.zeros((B,) + IMG, np.float32)
        x0, xt = np.zeros((n_max - 1, B) + IMG, np.float32), np.zeros((n_max - 1, B) + IMG, np.float32)
        for k, (nl, g, mix, hn) in enumerate(recs):
            v = e[k] * np.float32(0.5) + l[k, 0] + np.float32(g) + np.float32(0.125 * nl)
            if z is not None:
                v = v + np.float32(0.25 * mix) * z[k]
            if mm is not None:
                v = v + mm[k]
            if hn and ng is not None:
                v = v + ng[k, 1]
            val[k] = v
            for i in range(nl - 1):
                x0[i, k], xt[i, k] = v + np.float32(i + 1), v - np.float32(i + 1)
        self._arr(out, (B,) + IMG)[:] = val
        self.names.add(f"out{n}", val)
        for what, p, full in (("x0", tx0, x0), ("xt", txt, xt)):
            t = self._arr(p, (n_max - 1, B) + IMG)
            if t is not None:
                for k, r in enumerate(recs):
                    t[: r[0] - 1, k] = full[: r[0] - 1, k]
                self.names.add(f"{what}_{n}", full)
        self.log.append(dict(entry=entry, engine_batch=self.state["engine"], B=B, **scalars, noise=self.names.of(e), labels=self.names.of(l),
                             init=self.names.of(z), mask=self.names.of(mm), neg=self.names.of(ng), coeffs=coeffs,
                             trace=[self._arr(tx0, (1,)) is not None, self._arr(txt, (1,)) is not None],
                             stream=stream.value if isinstance(stream, C.c_void_p) else stream, writes=f"out{n}"))
        return 0

    def tld_sample(self, h, xT, lab, co, n_levels, g, sharp, bright, out, B, tx0, txt, stream):
        tab = np.ctypeslib.as_array(co, shape=(n_levels, 6))
        return self._run("tld_sample", B, xT, lab, None, None, None, [(n_levels, g, 1.0, 0)] * B, self.names.of(tab),
                         dict(n_levels=n_levels, class_guidance=g, sharp_f=sharp, bright_f=bright), out, tx0, txt, stream)

    def tld_sample_from(self, h, eps, z0, m, start_mix, lab, co, n_levels, g, sharp, bright, out, B, tx0, txt, stream):
        tab = np.ctypeslib.as_array(co, shape=(n_levels, 6))
        return self._run("tld_sample_from", B, eps, lab, z0, m, None, [(n_levels, g, start_mix, 0)] * B, self.names.of(tab),
                         dict(n_levels=n_levels, class_guidance=g, start_mix=start_mix, sharp_f=sharp, bright_f=bright), out, tx0, txt, stream)

    def _requests(self, entry, eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream, **host):
        """The four requests entries.  ``host``: the entry's further HOST arrays by parameter name (a pointer or None) -- a guidance table is
        recorded as its values per request, the noise coefficients by name, the keys and the shape rows as values; a NULL as None."""
        recs = [(r.n_levels, r.class_guidance, r.start_mix, r.has_negative) for r in recs]
        tab = np.ctypeslib.as_array(table, shape=(B, n_max, 6))
        coeffs = [self.names.of(tab[k, : r[0]]) for k, r in enumerate(recs)]
        pad = all(not tab[k, r[0]:].any() for k, r in enumerate(recs))
        extra = {}
        for what, p in host.items():
            if p is None:
                extra[what] = None
            elif what == "noise_keys":
                extra[what] = [int(v) for v in np.ctypeslib.as_array(p, shape=(B,))]
            elif what == "shape":
                extra[what] = np.ctypeslib.as_array(p, shape=(B, 4)).astype(np.float64).tolist()
            else:
                t = np.ctypeslib.as_array(p, shape=(B, n_max))
                rows = [t[k, : r[0]] for k, r in enumerate(recs)]
                extra[what] = [self.names.of(v) for v in rows] if what == "noise_coeff" else [v.astype(np.float64).tolist() for v in rows]
                extra[what + "_padding_zero"] = all(not t[k, r[0]:].any() for k, r in enumerate(recs))
        return self._run(entry, B, eps, lab, z0, m, neg, recs, coeffs,
                         dict(n_max=n_max, sharp_f=sharp, bright_f=bright, records=[list(r) for r in recs], table_padding_zero=pad, **extra),
                         out, tx0, txt, stream)

    def tld_sample_requests(self, h, eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream):
        return self._requests("tld_sample_requests", eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream)

    def tld_sample_requests_guided(self, h, eps, z0, m, lab, neg, recs, table, guidance, n_max, sharp, bright, out, B, tx0, txt, stream):
        return self._requests("tld_sample_requests_guided", eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream, guidance=guidance)

    def tld_sample_requests_stochastic(self, h, eps, z0, m, lab, neg, recs, table, guidance, noise_coeff, noise_keys, n_max, sharp, bright, out, B, tx0, txt,
                                       stream):
        return self._requests("tld_sample_requests_stochastic", eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream,
                              guidance=guidance, noise_coeff=noise_coeff, noise_keys=noise_keys)

    def tld_sample_requests_shaped(self, h, eps, z0, m, lab, neg, recs, table, guidance, noise_coeff, noise_keys, shape, n_max, sharp, bright, out, B, tx0,
                                   txt, stream):
        return self._requests("tld_sample_requests_shaped", eps, z0, m, lab, neg, recs, table, n_max, sharp, bright, out, B, tx0, txt, stream,
                              guidance=guidance, noise_coeff=noise_coeff, noise_keys=noise_keys, shape=shape)


def _label(text):
    return torch.randn(TXT, generator=torch.Generator().manual_seed(sum((i + 1) * ord(c) for i, c in enumerate(text)))) * 0.5


class Vae:
    """decode: the first three channels, each latent cell repeated 8 x 8, 2 frac(x / 64) - 1 (exact in float32, inside [-1, 1)).  encode: 8 x 8 area average, channel 0 once more as
    the fourth channel; ``sample`` adds 0.1 x randn from the caller's generator."""
    dtype = torch.float32

    def __init__(self, names, log, state):
        self.names, self.log, self.state = names, log, state

    def _n(self):
        self.state["n"] += 1
        return self.state["n"] - 1

    def decode(self, x):
        src = "?"
        for s in (1, 2, 4, 8):
            nm = self.names.of(x / s)
            if "?" not in json.dumps(nm):
                src = nm if s == 1 else {"times": s, "of": nm}
                break
        y = x.float()[:, :3].repeat_interleave(8, 2).repeat_interleave(8, 3) / 64
        img = (y - y.floor()) * 2 - 1
        name = f"dec{self._n()}"
        self.names.add(name, img)
        self.log.append(dict(entry="vae.decode", input=src, dtype=str(x.dtype), writes=name))
        return (img.to(x.dtype),)

    def encode(self, x):
        n = self._n()
        pooled = torch.nn.functional.avg_pool2d(x.float(), 8)
        mode = torch.cat([pooled, pooled[:, :1]], 1)
        self.names.add(f"zmode{n}", mode)
        self.names.add(f"zmode{n}/8", mode / 8)
        self.log.append(dict(entry="vae.encode", input=self.names.of(x), dtype=str(x.dtype), writes=f"zmode{n}"))
        vae = self

        class Dist:
            def mode(self):
                vae.log.append(dict(entry="latent_dist.mode"))
                return mode

            def sample(self, generator=None):
                z = mode + 0.1 * torch.randn(mode.shape, generator=generator)
                vae.names.add(f"zsample{n}", z)
                vae.names.add(f"zsample{n}/8", z / 8)
                vae.log.append(dict(entry="latent_dist.sample", seed=generator.initial_seed(), writes=f"zsample{n}"))
                return z

        return type("Enc", (), {"latent_dist": Dist()})()


def build_transcript(mp):
    from transformer_latent_diffusion_amd import (Denoiser, DenoiserConfig, DiffusionGenerator, DiffusionTransformer, LTDConfig, RequestBatcher,
                                                  _lib, latent_mask, schedule, sharded)
    from transformer_latent_diffusion_amd.diffusion import make_image_grid
    names, log, state, out = Names(), [], {"n": 0, "engine": None}, []
    mp.setattr(_lib, "lib", lambda: Lib(names, log, state))
    mp.setattr(_lib, "check", lambda rc, what: log[-1].__setitem__("checked_as", what))
    mp.setattr(torch.cuda, "current_stream", lambda dev=None: type("S", (), {"cuda_stream": 7})())
    mp.setattr(torch.cuda, "device", lambda dev: contextlib.nullcontext())

    def fake(m):
        mp.setattr(m, "_resolve_device", lambda t=None: CPU)
        mp.setattr(m, "_ensure_engine", lambda n, dev: state.__setitem__("engine", n))
        return m

    def pil_name(p):
        got = np.asarray(p)
        quant = lambda t: (t.float().clip(0, 1).clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).numpy()
        for name, t in reversed(names.t):
            if name.startswith("dec"):
                pics = (torch.from_numpy(t) + 1) / 2
                for i in range(len(pics)):
                    if _same(quant(pics[i]), got):
                        return f"pil({name}[{i}])"
                if len(pics) > 1 and _same(quant(make_image_grid(pics, nrow=int(np.sqrt(len(pics))), padding=4)), got):
                    return f"pil(grid({name}))"
        return "?"

    def describe(r):
        if isinstance(r, Tensor):
            return dict(shape=list(r.shape), dtype=str(r.dtype), device=str(r.device), value=names.of(r))
        if isinstance(r, (tuple, list)):
            return [describe(v) for v in r]
        if isinstance(r, dict):
            return {str(k): describe(v) for k, v in r.items()}
        if hasattr(r, "convert"):
            return dict(pil=list(r.size), mode=r.mode, value=pil_name(r))
        return r

    def call(label, fn):
        start = len(log)
        try:
            r = dict(returns=describe(fn()))
        except Exception as exc:
            r = dict(raises=type(exc).__name__, message=str(exc))
            if hasattr(exc, "partial"):
                r["partial"] = describe(exc.partial)
        out.append(dict(call=label, **r, calls=log[start:]))

    # ---- the table of expected tensors ------------------------------------------------------------------------------------------------
    def randn(seed, B, dtype=torch.float32):
        x = torch.randn(B, CH, S, S, dtype=dtype, generator=torch.Generator(device="cpu").manual_seed(seed))
        return names.add(f"randn(seed {seed}, B {B}{'' if dtype == torch.float32 else ', bf16'})", x)

    LEVELS = [0.9, 0.7, 0.45, 0.2, 0.05]
    for n in (3, 4, 5, 6, 8, 15, 30):
        for e in (1, 2):
            for plus in (True, False):
                for s in (None, 0.65, 0.3):
                    lv = schedule.noise_schedule(n, e)
                    try:
                        if s is not None:
                            lv = schedule.truncate_levels(lv, s)[1]
                    except ValueError:
                        continue
                    names.add(f"coef(n {n}, e {e}, {'dpm' if plus else 'ddim'}{'' if s is None else f', s {s}'})", schedule.step_coefficients(lv, plus))
    for s in (None, 0.65):
        lv = schedule.noise_schedule(99, 1, LEVELS)
        names.add(f"coef(LEVELS{'' if s is None else f', s {s}'})", schedule.step_coefficients(lv if s is None else schedule.truncate_levels(lv, s)[1], True))
    for n in (3, 4, 5, 6, 8):                           # the stochastic solvers: the table and the noise coefficient per forward
        names.add(f"ecoef zeros {n}", np.zeros(n, np.float32))
        for plus in (True, False):
            for eta in (0.5, 1.0):
                co, e = schedule.step_coefficients(schedule.noise_schedule(n, 1), plus, eta)
                names.add(f"coef(n {n}, e 1, {'dpm' if plus else 'ddim'}, eta {eta})", co)
                names.add(f"ecoef(n {n}, e 1, {'dpm' if plus else 'ddim'}, eta {eta})", e)
    co, e = schedule.step_coefficients(schedule.truncate_levels(schedule.noise_schedule(8, 1), 0.65)[1], True, 1.0)
    names.add("coef(n 8, e 1, dpm, s 0.65, eta 1.0)", co)
    names.add("ecoef(n 8, e 1, dpm, s 0.65, eta 1.0)", e)
    names.add(f"ecoef zeros {co.shape[0]}", np.zeros(co.shape[0], np.float32))
    rg = torch.Generator().manual_seed(61)
    eps5, z5 = torch.randn(5, CH, S, S, generator=rg), torch.randn(5, CH, S, S, generator=rg) * 0.5
    lab5, neg5 = torch.randn(5, TXT, generator=rg) * 0.5, torch.randn(5, TXT, generator=rg) * 0.5
    mask5 = torch.zeros(5, 1, S, S)
    mask5[:, :, 5:13, 3:9] = 1
    mask5[4] = torch.rand(1, S, S, generator=rg)
    for nm, t in (("eps5", eps5), ("z5", z5), ("lab5", lab5), ("neg5", neg5), ("mask5", mask5)):
        names.add(nm, t)
    names.add("z5 rows 1, 3, else zeros", torch.stack([torch.zeros(IMG), z5[1], torch.zeros(IMG), z5[3], torch.zeros(IMG)]))
    names.add("mask5 row 3, else ones", torch.stack([torch.ones(1, S, S)] * 3 + [mask5[3], torch.ones(1, S, S)]))
    names.add("neg5 rows 1, 4, else zeros", torch.stack([torch.zeros(TXT), neg5[1], torch.zeros(TXT), torch.zeros(TXT), neg5[4]]))
    for seed, B in ((10, 16), (10, 5), (10, 3), (4, 5), (11, 1), (12, 1), (13, 1), (14, 1), (21, 1), (22, 1), (23, 1), (3, 1), (5, 4), (9, 1), (6, 1)):
        randn(seed, B)
    randn(10, 3, torch.bfloat16)

    vae = Vae(names, log, state)
    m = fake(Denoiser(**asdict(DenoiserConfig(n_channels=4))))
    gen, gen0 = DiffusionGenerator(m, vae, CPU, torch.float32), DiffusionGenerator(m, None, CPU, torch.float32)
    genb = DiffusionGenerator(m, vae, CPU, torch.bfloat16)
    lab16 = names.add("lab16", torch.randn(16, TXT, generator=rg) * 0.5)
    five = dict(class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], n_iter=[8, 5, 8, 3, 5], use_ddpm_plus=[True, True, False, True, True], exponent=[1, 1, 1, 1, 2])
    neg_list, z_list, m_list = [None, neg5[1], None, None, neg5[4]], [None, z5[1], None, z5[3], None], [None, None, None, mask5[3], None]

    # ---- generate, generate_latents ---------------------------------------------------------------------------------------------------
    call("generate defaults", lambda: gen.generate(lab16, img_size=S))
    call("generate int seed, scale 4", lambda: gen.generate(lab5, n_iter=8, num_imgs=5, class_guidance=4.5, seed=4, scale_factor=4, img_size=S))
    call("generate seeds tensor, DDIM", lambda: gen.generate(lab5, n_iter=6, num_imgs=5, seeds=eps5, img_size=S, use_ddpm_plus=False, sharp_f=0, bright_f=0.25))
    call("generate noise_levels, exponent ignored", lambda: gen.generate(lab5[:3], n_iter=99, num_imgs=3, img_size=S, noise_levels=LEVELS))
    call("generate vae None", lambda: gen0.generate(lab5[:3], n_iter=5, num_imgs=3, img_size=S, exponent=2))
    call("generate bf16 model dtype", lambda: genb.generate(lab5[:3], n_iter=5, num_imgs=3, img_size=S))
    call("generate_latents trace", lambda: gen.generate_latents(lab5, n_iter=8, num_imgs=5, class_guidance=3.0, seeds=eps5, img_size=S, trace=True))
    call("generate_latents bf16 trace", lambda: genb.generate_latents(lab5[:3], n_iter=4, num_imgs=3, img_size=S, trace=True))
    call("generate_latents empty", lambda: gen.generate_latents(lab5[:0], n_iter=4, num_imgs=0, img_size=S, trace=True))
    # ---- generate_from, generate_latents_from ------------------------------------------------------------------------------------------
    call("generate_from strength 1.0", lambda: gen.generate_from(z5, lab5, strength=1.0, n_iter=8))
    call("generate_from strength 0.65", lambda: gen.generate_from(z5, lab5, strength=0.65, n_iter=8, seed=4, scale_factor=4))
    call("generate_from defaults, vae None", lambda: gen0.generate_from(z5[:3], lab5[:3]))
    call("generate_from mask", lambda: gen.generate_from(z5, lab5, strength=0.65, mask=mask5, n_iter=8, seeds=eps5, use_ddpm_plus=False))
    call("generate_latents_from trace, noise_levels", lambda: gen.generate_latents_from(z5, lab5, strength=0.65, mask=mask5, n_iter=99, seeds=eps5,
                                                                                      noise_levels=LEVELS, trace=True))
    call("generate_latents_from bf16", lambda: genb.generate_latents_from(z5[:3], lab5[:3], strength=0.3, n_iter=15, exponent=2))
    call("generate_latents_from empty", lambda: gen.generate_latents_from(z5[:0], lab5[:0], trace=True))
    # ---- generate_latents_requests, generate_requests ----------------------------------------------------------------------------------
    call("requests five mixed, trace", lambda: gen.generate_latents_requests(lab5, seeds=eps5, img_size=S, trace=True, **five))
    call("requests negatives tensor", lambda: gen.generate_latents_requests(lab5, negative_labels=neg5, n_iter=[4, 6, 5, 6, 3], class_guidance=2.0))
    call("requests negatives list, int seeds", lambda: gen.generate_latents_requests(lab5, negative_labels=neg_list, seeds=[11, 12, 13, 14, 11],
                                                                                     n_iter=[3, 8, 4, 8, 5], sharp_f=0, bright_f=0))
    call("requests init and mask lists", lambda: gen.generate_latents_requests(lab5, init_latents=z_list, mask=m_list, strength=[None, 0.65, 1.0, 0.3, None],
                                                                               n_iter=[8, 8, 5, 15, 4], seed=4, trace=True))
    call("requests init tensor, scalar strength", lambda: gen.generate_latents_requests(lab5, init_latents=z5, strength=0.65, mask=mask5, n_iter=8,
                                                                                        negative_labels=neg_list, noise_levels=None))
    call("requests noise_levels", lambda: gen.generate_latents_requests(lab5[:3], noise_levels=LEVELS, n_iter=[1, 2, 3], init_latents=z5[:3],
                                                                        strength=[0.65, None, None]))
    call("requests all-None lists", lambda: gen.generate_latents_requests(lab5[:3], negative_labels=[None] * 3, init_latents=[None] * 3, mask=[None] * 3, n_iter=4))
    call("requests bf16, trace", lambda: genb.generate_latents_requests(lab5[:3], n_iter=[4, 5, 4], trace=True))
    call("requests B = 0", lambda: gen.generate_latents_requests(lab5[:0], n_iter=4, trace=True))
    call("requests B = 0, int seeds", lambda: gen.generate_latents_requests(lab5[:0], n_iter=[], seeds=[]))
    call("generate_requests five mixed", lambda: gen.generate_requests(lab5, seeds=eps5, img_size=S, trace=True, **five))
    call("generate_requests scale 4, negatives", lambda: gen.generate_requests(lab5, scale_factor=4, negative_labels=neg_list, n_iter=[5, 4, 3, 4, 5]))
    call("generate_requests vae None", lambda: gen0.generate_requests(lab5[:3], n_iter=4))
    call("generate_requests B = 0", lambda: gen.generate_requests(lab5[:0], n_iter=4))
    # ---- Denoiser.sample_latents* directly ------------------------------------------------------------------------------------------------
    co8, co5 = schedule.step_coefficients(schedule.noise_schedule(8, 1)), schedule.step_coefficients(schedule.noise_schedule(5, 1))
    call("sample_latents float64 coefficients", lambda: m.sample_latents(eps5.double(), lab5.double(), co8.astype(np.float64), 3, trace=True))
    call("sample_latents_from", lambda: m.sample_latents_from(eps5, z5, lab5, co5, 2.5, 0.75, mask=mask5, sharp_f=0.5))
    call("sample_latents_requests", lambda: m.sample_latents_requests(eps5, lab5, [co5, co8, co5, co8, co5], [1, 2, 3, 4, 5], neg_labels=neg_list, init_latents=z5,
                                                                      start_mix=[1, 0.5, 1, 0.25, 1], mask=mask5, sharp_f=0.5, bright_f=0.25, trace=True))
    # ---- the sharded wrappers, no process group ------------------------------------------------------------------------------------------
    call("generate_latents_sharded", lambda: sharded.generate_latents_sharded(gen, lab5, n_iter=6, num_imgs=5, class_guidance=4.5, seed=4, img_size=S,
                                                                              sharp_f=0.25, bright_f=0, exponent=2, use_ddpm_plus=False))
    call("generate_latents_sharded seeds, noise_levels", lambda: sharded.generate_latents_sharded(gen, lab5, num_imgs=5, seeds=eps5, img_size=S, noise_levels=LEVELS))
    call("generate_latents_from_sharded", lambda: sharded.generate_latents_from_sharded(gen, z5, lab5, strength=0.65, mask=mask5, n_iter=8, seed=4))
    call("generate_latents_from_sharded defaults", lambda: sharded.generate_latents_from_sharded(genb, z5[:3], lab5[:3]))
    call("generate_latents_requests_sharded five mixed", lambda: sharded.generate_latents_requests_sharded(gen, lab5, seeds=eps5, img_size=S, **five))
    call("generate_latents_requests_sharded lists", lambda: sharded.generate_latents_requests_sharded(
        gen, lab5, seeds=[11, 12, 13, 14, 11], negative_labels=neg_list, init_latents=z_list, mask=m_list, strength=[None, 0.65, 1.0, 0.3, None],
        n_iter=[8, 8, 5, 15, 4], class_guidance=[1.0, 2.0, 3.0, 4.0, 5.0], sharp_f=0))
    call("generate_latents_requests_sharded tensors, seed", lambda: sharded.generate_latents_requests_sharded(
        gen, lab5, seed=4, negative_labels=neg5, init_latents=z5, mask=mask5, strength=0.65, n_iter=8))

    # ---- DiffusionTransformer: stand-in text encoder and VAE -------------------------------------------------------------------------------
    def text_encoder(prompts):
        log.append(dict(entry="text_encoder", texts=list(prompts)))
        if "boom" in prompts:
            raise RuntimeError("the encoder failed on 'boom'")
        return torch.stack([names.add(f"L({p})", _label(p)) for p in prompts])

    class Tok:
        def tokenize(self, prompts, truncate=False):
            log.append(dict(entry="tokenize", texts=list(prompts), truncate=truncate))
            return torch.tensor([[ord(c) for c in p.ljust(8)[:8]] for p in prompts])

    class Clip:
        def encode_text(self, tokens):
            texts = ["".join(chr(int(c)) for c in row).rstrip() for row in tokens]
            log.append(dict(entry="clip.encode_text", texts=texts, device=str(tokens.device)))
            return torch.stack([names.add(f"L({p})", _label(p)) for p in texts])

    cfg = LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4))
    pipe = DiffusionTransformer(cfg, vae=vae, text_encoder=text_encoder, run_device=CPU)
    pipec = DiffusionTransformer(cfg, vae=vae, clip_model=Clip(), tokenizer=Tok(), run_device=CPU)
    fake(pipe.diffuser.model), fake(pipec.diffuser.model)
    for tag, p in (("text_encoder: ", pipe), ("clip_model: ", pipec)):
        call(tag + "encode_text", lambda: p.encode_text(["cat", "dog"]))
        call(tag + "images_from_texts scalars", lambda: p.generate_images_from_texts(["cat", "dog", "owl"], class_guidance=4.5, seeds=11, n_iter=5))
        call(tag + "images_from_texts per prompt", lambda: p.generate_images_from_texts(["cat", "dog", "owl"], class_guidance=[1.0, 6, 3.0], seeds=[13, 12, 11], n_iter=[4, 8, 4]))
        call(tag + "images_from_texts negatives", lambda: p.generate_images_from_texts(["cat", "dog", "owl"], seeds=[21, 22, 23], negative_prompts=[None, "blurry", None]))
        call(tag + "images_from_texts one negative for all", lambda: p.generate_images_from_texts(["cat", "dog"], n_iter=[4, 5], negative_prompts="blurry"))
        call(tag + "image_from_text", lambda: p.generate_image_from_text("cat", n_iter=5))
        call(tag + "image_from_text negative", lambda: p.generate_image_from_text("cat", seed=3, n_iter=5, negative_prompt="blurry"))
    call("images_from_texts defaults", lambda: pipe.generate_images_from_texts(("cat", "dog")))
    call("images_from_texts all-None negatives", lambda: pipe.generate_images_from_texts(["cat"], negative_prompts=[None]))
    call("images_from_texts no prompts", lambda: pipe.generate_images_from_texts([], class_guidance=[1.0]))
    call("image_from_text grid of four", lambda: pipe.generate_image_from_text("owl", class_guidance=3, seed=5, num_imgs=4, img_size=99))
    call("image_from_text grid of four, negative", lambda: pipe.generate_image_from_text("owl", seed=5, num_imgs=4, negative_prompt="dim"))
    image = torch.rand(3, 8 * S, 8 * S, generator=rg)
    names.add("2 image - 1", (image * 2 - 1).unsqueeze(0))
    names.add("white image", torch.ones(1, 3, 8 * S, 8 * S))
    pmask = torch.zeros(8 * S, 8 * S)
    pmask[40:96, 17:80] = 1
    names.add("latent_mask(pmask)", latent_mask(pmask, S).unsqueeze(0))
    call("image_from_image", lambda: pipe.generate_image_from_image(image, "cat", seed=9, n_iter=8))
    call("image_from_image mask, latents", lambda: pipe.generate_image_from_image(image, "cat", strength=0.65, mask=pmask, seed=9, n_iter=8, return_latents=True))
    call("image_from_image negative, posterior", lambda: pipe.generate_image_from_image(image, "cat", strength=0.3, mask=pmask.unsqueeze(0), class_guidance=3, seed=6,
                                                                                        n_iter=15, sample_posterior=True, return_latents=True, negative_prompt="blurry"))
    call("image_from_image PIL image and mask", lambda: pipec.generate_image_from_image(
        __import__("PIL.Image").Image.fromarray(np.full((8 * S, 8 * S, 3), 255, np.uint8)), "dog", seed=9, n_iter=4,
        mask=__import__("PIL.Image").Image.fromarray(np.full((8 * S, 8 * S), 255, np.uint8))))
    call("latent_mask", lambda: latent_mask(pmask, S))

    # ---- RequestBatcher --------------------------------------------------------------------------------------------------------------------
    def batcher(mixed, prompts):
        rb = RequestBatcher(pipe, max_batch=2, mixed=mixed)
        subs = [("cat", 6, 11, 4), ("dog", 3, 12, 4), ("owl", 6, 13, 4), (prompts, 6, 14, 5), ("cat", 6, 21, 4)]
        tickets = [rb.submit(*s) for s in subs]
        if mixed:
            tickets.append(rb.submit("dog", 2, 22, 3, negative_prompt="blurry"))
        res = [dict(tickets=tickets, pending=rb.pending(), plan=describe(rb.plan()))]
        try:
            res.append(describe(rb.flush()))
        except Exception as exc:
            res.append(dict(raises=type(exc).__name__, message=str(exc), partial=describe(exc.partial)))
        res.append(dict(pending=rb.pending(), plan=describe(rb.plan())))
        return res

    for mixed in (False, True):
        call(f"RequestBatcher mixed={mixed}", lambda: batcher(mixed, "fox"))
        call(f"RequestBatcher mixed={mixed}, a failing call", lambda: batcher(mixed, "boom"))
    call("RequestBatcher.call_rows", lambda: RequestBatcher.call_rows([(15, False), (30, True)]))

    # ---- refusals: type and message --------------------------------------------------------------------------------------------------------
    z3, l3, e3, k3 = z5[:3], lab5[:3], eps5[:3], mask5[:3]
    ok = dict(n_iter=[4, 5, 6], class_guidance=3.0, seed=1)
    co4n = schedule.step_coefficients(schedule.noise_schedule(4, 1)).shape[0]
    refusals = {
        "generate_latents labels batch": lambda: gen.generate_latents(l3, num_imgs=5, img_size=S),
        "generate labels batch": lambda: gen.generate(l3, seeds=eps5),
        "from init dim": lambda: gen.generate_latents_from(z3[0], l3),
        "from init vs noise": lambda: gen.generate_latents_from(z3, l3, num_imgs=4),
        "from init vs seeds": lambda: gen.generate_from(z3, l3, seeds=eps5),
        "from labels batch": lambda: gen.generate_latents_from(z3, lab5),
        "from mask shape": lambda: gen.generate_latents_from(z3, l3, mask=mask5),
        "from mask range": lambda: gen.generate_latents_from(z3, l3, mask=k3 * 2),
        "from mask negative": lambda: gen.generate_latents_from(z3, l3, mask=k3 - 0.5),
        "from strength": lambda: gen.generate_latents_from(z3, l3, strength=1.5),
        "from strength too low": lambda: gen.generate_latents_from(z3, l3, strength=0.01, n_iter=4),
        "requests n_iter count": lambda: gen.generate_latents_requests(l3, **dict(ok, n_iter=[4, 5])),
        "requests guidance count": lambda: gen.generate_latents_requests(l3, **dict(ok, class_guidance=[1.0, 2.0])),
        "requests exponent count": lambda: gen.generate_latents_requests(l3, **dict(ok, exponent=[1, 2])),
        "requests use_ddpm_plus count": lambda: gen.generate_latents_requests(l3, **dict(ok, use_ddpm_plus=[True])),
        "requests strength count": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, strength=[0.5] * 4)),
        "requests seeds count": lambda: gen.generate_latents_requests(l3, **dict(ok, seeds=[1, 2])),
        "requests seeds tensor batch": lambda: gen.generate_latents_requests(l3, **dict(ok, seeds=eps5)),
        "requests n_iter below 2": lambda: gen.generate_latents_requests(l3, **dict(ok, n_iter=[4, 1, 6])),
        "requests guidance nan": lambda: gen.generate_latents_requests(l3, **dict(ok, class_guidance=[1.0, float("nan"), 2.0])),
        "requests guidance inf": lambda: gen.generate_latents_requests(l3, **dict(ok, class_guidance=float("inf"))),
        "requests negatives width": lambda: gen.generate_latents_requests(l3, **dict(ok, negative_labels=torch.zeros(3, 767))),
        "requests negatives batch": lambda: gen.generate_latents_requests(l3, **dict(ok, negative_labels=torch.zeros(2, 768))),
        "requests negatives row": lambda: gen.generate_latents_requests(l3, **dict(ok, negative_labels=[None, torch.zeros(5), None])),
        "requests negatives count": lambda: gen.generate_latents_requests(l3, **dict(ok, negative_labels=[None, None])),
        "requests strength without init": lambda: gen.generate_latents_requests(l3, **dict(ok, strength=[None, 0.5, None])),
        "requests mask without init": lambda: gen.generate_latents_requests(l3, **dict(ok, mask=k3)),
        "requests strength range": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, strength=[0.5, 1.5, None])),
        "requests init batch": lambda: gen.generate_latents_requests(l3, **dict(ok, init_latents=z5[:2])),
        "requests init list count": lambda: gen.generate_latents_requests(l3, **dict(ok, init_latents=[None, z5[0]])),
        "requests init list entry": lambda: gen.generate_latents_requests(l3, **dict(ok, init_latents=[None, z5[0, :2], None])),
        "requests mask tensor shape": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, mask=torch.ones(3, 1, 8, 8))),
        "requests mask list entry": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, mask=[None, torch.ones(S, S), None])),
        "requests mask range": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, mask=torch.full((3, 1, S, S), 2.0))),
        "requests mask list range": lambda: gen.generate_latents_requests(l3, init_latents=z3, **dict(ok, mask=[None, torch.full((1, S, S), -1.0), None])),
        "requests img_size": lambda: gen.generate_latents_requests(l3, **dict(ok, img_size=8)),
        "generate_requests guidance count": lambda: gen.generate_requests(l3, **dict(ok, class_guidance=[1.0, 2.0])),
        "requests row cap": lambda: gen.generate_latents_requests(torch.zeros(40, TXT), n_iter=list(range(40, 80)), use_ddpm_plus=False),
        "sample_from init shape": lambda: m.sample_latents_from(e3, z5, l3, co5, 3.0, 1.0),
        "sample_from mask shape": lambda: m.sample_latents_from(e3, z3, l3, co5, 3.0, 1.0, mask=mask5),
        "sample_from mask shape, empty batch": lambda: m.sample_latents_from(e3[:0], z3[:0], l3[:0], co5, 3.0, 1.0, mask=k3),
        "sample_requests noise shape": lambda: m.sample_latents_requests(e3[:, :3], l3, [co5] * 3, [1.0] * 3),
        "sample_requests noise dim": lambda: m.sample_latents_requests(e3[0], l3, [co5] * 3, [1.0] * 3),
        "sample_requests labels shape": lambda: m.sample_latents_requests(e3, lab5, [co5] * 3, [1.0] * 3),
        "sample_requests coeff count": lambda: m.sample_latents_requests(e3, l3, [co5] * 2, [1.0] * 3),
        "sample_requests guidance count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 2),
        "sample_requests start_mix count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, start_mix=[1.0]),
        "sample_requests coeff shape": lambda: m.sample_latents_requests(e3, l3, [co5, co5[:1], co5], [1.0] * 3),
        "sample_requests coeff columns": lambda: m.sample_latents_requests(e3, l3, [co5, co5, co5[:, :5]], [1.0] * 3),
        "sample_requests guidance nan": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0, 2.0, float("nan")]),
        "sample_requests start_mix zero": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, start_mix=[1.0, 0.0, 1.0], init_latents=z3),
        "sample_requests start_mix above 1": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, start_mix=[1.0, 1.0, 1.5], init_latents=z3),
        "sample_requests init shape": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, init_latents=z5),
        "sample_requests start_mix without init": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, start_mix=[1.0, 0.5, 1.0]),
        "sample_requests mask without init": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, mask=k3),
        "sample_requests mask shape": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, init_latents=z3, mask=mask5),
        "sample_requests neg tensor shape": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, neg_labels=torch.zeros(3, 5)),
        "sample_requests neg count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, neg_labels=[None]),
        "sample_requests neg row": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, neg_labels=[None, torch.zeros(5), None]),
        "sample_requests bad neg row, empty batch": lambda: m.sample_latents_requests(e3[:0], l3[:0], [], [], neg_labels=torch.zeros(1, TXT)),
        "requests guidance_interval order": lambda: gen.generate_latents_requests(l3, **dict(ok, guidance_interval=(0.8, 0.3))),
        "requests guidance_interval count": lambda: gen.generate_latents_requests(l3, **dict(ok, guidance_interval=[None, (0.2, 0.9)])),
        "requests guidance_schedule count": lambda: gen.generate_latents_requests(l3, **dict(ok, guidance_schedule=[None, None])),
        "requests guidance_schedule length": lambda: gen.generate_latents_requests(l3, **dict(ok, guidance_schedule=[None, np.ones(2), None])),
        "requests guidance_schedule nan": lambda: gen.generate_latents_requests(l3, **dict(ok, n_iter=4, guidance_schedule=[None, np.full(co4n, float("nan")), None])),
        "requests eta negative": lambda: gen.generate_latents_requests(l3, **dict(ok, eta=[0.0, -0.5, 0.0])),
        "requests eta count": lambda: gen.generate_latents_requests(l3, **dict(ok, eta=[0.5, 0.5])),
        "requests eta with a seeds tensor": lambda: gen.generate_latents_requests(l3, **dict(ok, eta=0.5, seeds=e3)),
        "requests noise_seeds count": lambda: gen.generate_latents_requests(l3, **dict(ok, eta=0.5, noise_seeds=[1, 2])),
        "requests guidance_rescale range": lambda: gen.generate_latents_requests(l3, **dict(ok, guidance_rescale=1.5)),
        "requests apg_momentum range": lambda: gen.generate_latents_requests(l3, **dict(ok, apg_momentum=[0.0, 1.0, 0.0])),
        "requests apg_norm count": lambda: gen.generate_latents_requests(l3, **dict(ok, apg_norm=[1.0, 2.0])),
        "generate_latents eta nan": lambda: gen.generate_latents(l3, num_imgs=3, img_size=S, eta=float("nan")),
        "generate_latents_from apg_eta negative": lambda: gen.generate_latents_from(z3, l3, apg_eta=-1.0),
        "sample_requests guidance_steps count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, None, guidance_steps=[np.ones(5)] * 2),
        "sample_requests guidance_steps length": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, None, guidance_steps=[np.ones(co5.shape[0] + 1)] * 3),
        "sample_requests guidance_steps inf": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, None, guidance_steps=[np.full(co5.shape[0], float("inf"))] * 3),
        "sample_requests noise_coeffs without keys": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, noise_coeffs=[np.zeros(co5.shape[0])] * 3),
        "sample_requests noise_keys count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, noise_coeffs=[np.zeros(co5.shape[0])] * 3, noise_keys=[1]),
        "sample_requests noise_coeffs final": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, noise_coeffs=[np.ones(co5.shape[0])] * 3, noise_keys=[1, 2, 3]),
        "sample_requests noise_keys range": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, noise_coeffs=[np.zeros(co5.shape[0])] * 3, noise_keys=[1, -2, 3]),
        "sample_requests shape count": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, shape=[(1.0, 0.0, 0.0, 0.0)] * 2),
        "sample_requests shape row": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, shape=[(1.0, 0.0, 0.0)] * 3),
        "sample_requests shape phi": lambda: m.sample_latents_requests(e3, l3, [co5] * 3, [1.0] * 3, shape=[(1.0, 0.0, 0.0, 2.0)] * 3),
        "latent_mask not square": lambda: latent_mask(torch.zeros(32, 16), 16),
        "latent_mask dims": lambda: latent_mask(torch.zeros(2, 32, 32), 16),
        "latent_mask multiple": lambda: latent_mask(torch.zeros(1, 40, 40), 16),
        "latent_mask latent size": lambda: latent_mask(torch.zeros(40, 40), 0),
        "latent_mask range": lambda: latent_mask(torch.full((32, 32), 1.5), 16),
        "texts seeds count": lambda: pipe.generate_images_from_texts(["cat", "dog"], seeds=[1]),
        "texts seeds count, per prompt": lambda: pipe.generate_images_from_texts(["cat", "dog"], class_guidance=[1, 2], seeds=[1, 2, 3]),
        "texts guidance count": lambda: pipe.generate_images_from_texts(["cat", "dog"], class_guidance=[1.0]),
        "texts n_iter count": lambda: pipe.generate_images_from_texts(["cat", "dog"], n_iter=[4, 5, 6]),
        "texts negatives count": lambda: pipe.generate_images_from_texts(["cat", "dog"], negative_prompts=["blurry"]),
        "texts n_iter below 2": lambda: pipe.generate_images_from_texts(["cat", "dog"], n_iter=[4, 1]),
        "image not an image": lambda: pipe.generate_image_from_image([[0.5]], "cat"),
        "image shape": lambda: pipe.generate_image_from_image(torch.zeros(3, 64, 64), "cat"),
        "image dims": lambda: pipe.generate_image_from_image(torch.zeros(1, 3, 8 * S, 8 * S), "cat"),
        "image range": lambda: pipe.generate_image_from_image(image * 2, "cat"),
        "image mask side": lambda: pipe.generate_image_from_image(image, "cat", mask=torch.zeros(64, 64)),
        "image mask range": lambda: pipe.generate_image_from_image(image, "cat", mask=pmask * 3),
        "image strength": lambda: pipe.generate_image_from_image(image, "cat", strength=0.0),
        "batcher negative prompt": lambda: RequestBatcher(pipe).submit("cat", negative_prompt="blurry"),
        "sharded from init vs noise": lambda: sharded.generate_latents_from_sharded(gen, z3, l3, num_imgs=4),
        "sharded from mask batch": lambda: sharded.generate_latents_from_sharded(gen, z3, l3, mask=mask5),
        "sharded requests init batch": lambda: sharded.generate_latents_requests_sharded(gen, l3, init_latents=z5, n_iter=4),
        "sharded requests mask without init": lambda: sharded.generate_latents_requests_sharded(gen, l3, mask=[None, k3[0], None], n_iter=4),
        "sharded requests n_iter count": lambda: sharded.generate_latents_requests_sharded(gen, l3, n_iter=[4, 5]),
        "sharded_sample extras": lambda: sharded.sharded_sample(lambda *a: a[0], e3, l3, extras=(None, z5)),
        "Denoiser.train": lambda: m.train(),
        "Denoiser.to dtype": lambda: m.to(torch.float64),
        "Denoiser.set_low_latency": lambda: m.set_low_latency(3),
        "Denoiser.load_state_dict unexpected": lambda: m.load_state_dict(dict(m.state_dict(), zzz=torch.zeros(1))),
        "Denoiser.forward x shape": lambda: m(e3[:, :, :8], torch.zeros(3, 1), l3),
        "Denoiser.forward label shape": lambda: m(e3, torch.zeros(3, 1), lab5),
        "Denoiser.forward dtype": lambda: m(e3.double(), torch.zeros(3, 1), l3),
        "Denoiser without a device": lambda: Denoiser(**asdict(DenoiserConfig(n_channels=4)))(e3, torch.zeros(3, 1), l3),
    }
    for label, fn in refusals.items():
        call("refusal: " + label, fn)
    # ---- the guided, stochastic and shaped entries through the public API (after every older call: the stand-in numbers what it writes) --------------------------------------------------------------------
    ge = dict(n_iter=[8, 5, 8, 3, 5], class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], seeds=[11, 12, 13, 14, 11])
    n8, n5 = co8.shape[0], co5.shape[0]
    call("requests guidance_interval for all, trace", lambda: gen.generate_latents_requests(lab5, guidance_interval=(0.3, 0.8), trace=True, **ge))
    call("requests guidance_interval per request", lambda: gen.generate_latents_requests(lab5, guidance_interval=[None, (0.2, 0.9), (0.5, 0.5), None, (0.0, 1.0)],
                                                                                         negative_labels=neg_list, **ge))
    call("requests guidance_schedule", lambda: gen.generate_latents_requests(
        lab5[:3], n_iter=[8, 5, 8], class_guidance=2.0, seeds=[11, 12, 13], guidance_schedule=[np.linspace(4.0, 1.0, n8), None, np.ones(n8)]))
    call("requests guidance_schedule and interval", lambda: gen.generate_latents_requests(
        lab5[:3], n_iter=[5, 8, 5], class_guidance=2.0, seed=4, guidance_schedule=[None, np.full(n8, 1.5), None], guidance_interval=[(0.3, 0.8), None, None]))
    call("requests eta per request", lambda: gen.generate_latents_requests(lab5, eta=[0.0, 1.0, 0.5, 0.0, 1.0], use_ddpm_plus=[True, True, False, True, False], **ge))
    call("requests eta, batch seed", lambda: gen.generate_latents_requests(lab5[:3], n_iter=[4, 6, 4], eta=0.5, seed=4))
    call("requests eta, seeds tensor and noise_seeds", lambda: gen.generate_latents_requests(lab5, n_iter=5, eta=1.0, seeds=eps5, img_size=S,
                                                                                             noise_seeds=[1, 2, 1 << 40, (1 << 64) - 1, 5]))
    call("requests eta, init and mask", lambda: gen.generate_latents_requests(lab5, init_latents=z5, strength=0.65, mask=mask5, n_iter=8, eta=1.0, seed=4, trace=True))
    call("requests guidance_rescale", lambda: gen.generate_latents_requests(lab5, guidance_rescale=0.75, **ge))
    call("requests apg per request", lambda: gen.generate_latents_requests(lab5, apg_eta=[1.0, 0.0, 0.5, 1.0, 0.0], apg_norm=[0.0, 2.5, 0.0, 0.0, 15.0],
                                                                           apg_momentum=[0.0, -0.5, 0.0, 0.0, -0.75], guidance_rescale=[0.0, 0.0, 0.5, 0.0, 0.25], **ge))
    call("requests interval and eta", lambda: gen.generate_latents_requests(lab5, guidance_interval=(0.3, 0.8), eta=[1.0, 0.0, 0.5, 1.0, 0.0], **ge))
    call("requests interval and shape", lambda: gen.generate_latents_requests(lab5, guidance_interval=[None, (0.2, 0.9), None, None, (0.3, 0.8)], guidance_rescale=0.5,
                                                                              apg_norm=2.5, **ge))
    call("requests eta and shape", lambda: gen.generate_latents_requests(lab5, eta=0.5, apg_eta=0.0, apg_momentum=-0.5, negative_labels=neg5, **ge))
    call("requests interval, eta and shape, trace", lambda: gen.generate_latents_requests(lab5, guidance_interval=(0.3, 0.8), eta=[1.0, 0.0, 0.5, 1.0, 0.0],
                                                                                          guidance_rescale=[0.5, 0.0, 0.0, 0.25, 0.0], trace=True, **ge))
    call("generate_latents guidance_interval", lambda: gen.generate_latents(lab5, n_iter=8, num_imgs=5, class_guidance=3.0, seed=4, img_size=S, guidance_interval=(0.3, 0.8)))
    call("generate_latents eta", lambda: gen.generate_latents(lab5[:3], n_iter=5, num_imgs=3, seed=4, img_size=S, eta=1.0, use_ddpm_plus=False))
    call("generate_latents apg, trace", lambda: gen.generate_latents(lab5[:3], n_iter=5, num_imgs=3, seed=4, img_size=S, apg_eta=0.0, apg_norm=2.5, trace=True))
    call("generate eta and rescale", lambda: gen.generate(lab5[:3], n_iter=5, num_imgs=3, seed=4, img_size=S, eta=0.5, guidance_rescale=0.75))
    call("generate_latents_from interval, eta, rescale, mask", lambda: gen.generate_latents_from(z5, lab5, strength=0.65, mask=mask5, n_iter=8, seed=4,
                                                                                                guidance_interval=(0.1, 0.5), eta=1.0, guidance_rescale=0.5))
    call("generate_from apg", lambda: gen.generate_from(z5[:3], lab5[:3], strength=1.0, n_iter=5, seed=4, apg_momentum=-0.5))
    g3s, e3s = [np.full(n5, 2.0), np.r_[np.ones(n8 - 1), 3.0], np.ones(n5)], [np.zeros(n5), np.r_[np.full(n8 - 1, 0.25), 0.0], np.zeros(n5)]
    names.add("e3s[1]", e3s[1])
    call("sample_latents_requests guidance_steps", lambda: m.sample_latents_requests(eps5[:3], lab5[:3], [co5, co8, co5], None, guidance_steps=g3s, trace=True))
    call("sample_latents_requests noise", lambda: m.sample_latents_requests(eps5[:3], lab5[:3], [co5, co8, co5], [1, 2, 3], noise_coeffs=e3s, noise_keys=[7, 8, 9]))
    call("sample_latents_requests shape alone", lambda: m.sample_latents_requests(eps5[:3], lab5[:3], [co5, co8, co5], [1, 2, 3],
                                                                                  shape=[(1.0, 0.0, 0.0, 0.0), (0.0, 2.5, -0.5, 0.0), (1.0, 0.0, 0.0, 0.5)]))
    call("sample_latents_requests steps, noise and shape", lambda: m.sample_latents_requests(
        eps5[:3], lab5[:3], [co5, co8, co5], None, guidance_steps=g3s, noise_coeffs=e3s, noise_keys=[7, 8, (1 << 64) - 1], shape=[(1.0, 0.0, 0.0, 0.5)] * 3,
        neg_labels=neg_list[:3], init_latents=z5[:3], start_mix=[1, 0.5, 1], mask=mask5[:3]))
    call("sample_latents_requests steps and shape, empty batch", lambda: m.sample_latents_requests(eps5[:0], lab5[:0], [], None, guidance_steps=[], shape=[], trace=True))
    text = json.dumps(out)
    assert '"?"' not in text, "a tensor the table does not name: " + next(json.dumps(c) for c in out if '"?"' in json.dumps(c))[:2000]
    bad = [c["call"] for c in out if ("raises" in c) != c["call"].startswith("refusal: ")]
    assert not bad, f"calls that should (not) have raised: {bad}"
    return json.loads(text)


def test_sampler_surface_transcript(monkeypatch):
    got = build_transcript(monkeypatch)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert [c["call"] for c in got] == [c["call"] for c in want]
    for g, w in zip(got, want):
        assert g == w, f"{w['call']}: the transcript differs\n got {json.dumps(g)[:3000]}\nwant {json.dumps(w)[:3000]}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import pytest
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_sampler_surface_host.py --record")
    with pytest.MonkeyPatch.context() as mp:
        doc = build_transcript(mp)
    with open(GOLDEN, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in doc) + "\n]\n")
    print(f"recorded {len(doc)} calls, {sum(len(c['calls']) for c in doc)} library / encoder / VAE calls -> {GOLDEN}")

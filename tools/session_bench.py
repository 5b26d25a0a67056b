#!/usr/bin/env python3
"""Sampler sessions beside the mixed request call, at BASELINE config C1 (100 M model, 256 px = 32 x 32 latents), in one process.

uniform leg   64 requests of 35 levels, guidance 6, admitted together into a 64-slot session: ms per step of the session (the 35 steps, and the
              admissions apart) beside ms per step of generate_latents_requests for the same 64 requests, with the time of every kernel class
              (HIP events, Denoiser.get_profile) for both.  The end latents are compared bitwise.
              --mixed-only times the mixed call alone: that form also runs on a tree that has no sessions yet (the baseline for "did the session
              cost the existing call anything").
trace leg     a fixed, seeded list of (arrival step, n_iter) pairs replayed through ContinuousBatcher(slots) and through RequestBatcher(mixed=True,
              max_batch=slots), which is flushed whenever it is idle.  Time is the measured time of the work itself (every step / flush is timed to
              its end, idle gaps are skipped, nothing sleeps); request k arrives at arrival_step[k] x --dt-ms.  Reports per-request latency (mean,
              p50, p95, ms) and the model-sample rows of each.  Small synthetic CLIP and VAE stand at the edges of both.
One JSON line at the end.
    python tools/session_bench.py [--leg uniform|trace|both] [--mixed-only] [--iters 5] [--slots 16] [--requests 48] [--seed 7] [--dt-ms 6] [--json out.json]"""
import argparse
import json
import os
import sys
import time
from dataclasses import asdict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator, _lib, config_100m  # noqa: E402
from transformer_latent_diffusion_amd.weights import synth_state_dict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--leg", default="both", choices=("uniform", "trace", "both"))
ap.add_argument("--mixed-only", action="store_true")
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--slots", type=int, default=16)
ap.add_argument("--requests", type=int, default=48)
ap.add_argument("--seed", type=int, default=7)
ap.add_argument("--dt-ms", type=float, default=6.0)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = torch.device("cuda", 0)
cfg = config_100m(32)
sd = {k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(cfg, 5).items()}
S, B, N = 32, 64, 35
res = {"config": "C1 100M 256px", "iters": args.iters}
median = lambda ts: sorted(ts)[len(ts) // 2]


def class_times(m, run):
    """ms per kernel class of one run (events around every launch of the class)."""
    m.set_profile(_lib.KERNEL_CLASSES)
    run()
    out = {c: round(m.get_profile(c)[0], 3) for c in _lib.KERNEL_CLASSES}
    m.set_profile(())
    return out


if args.leg in ("uniform", "both"):
    m = Denoiser(**asdict(cfg)).to(dev)
    m.load_state_dict(sd)
    m.reserve(2 * B)
    gen = DiffusionGenerator(m, None, dev, torch.float32)
    rng = torch.Generator().manual_seed(11)
    eps = torch.randn(B, 4, S, S, generator=rng).to(dev)
    labels = (torch.randn(B, 768, generator=rng) * 0.5).to(dev)
    kw = dict(sharp_f=0.0, bright_f=0.0, exponent=1)

    def mixed():
        return gen.generate_latents_requests(labels, n_iter=N, class_guidance=6, seeds=eps, **kw)

    want = mixed(); torch.cuda.synchronize()
    ts = []
    for _ in range(args.iters):
        t0 = time.perf_counter(); mixed(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
    t_mixed = median(ts)
    res["mixed_call"] = {"ms": round(t_mixed * 1e3, 2), "ms_per_step": round(t_mixed * 1e3 / N, 3), "ms_all": [round(v * 1e3, 2) for v in ts],
                         "classes_ms": class_times(m, mixed)}
    print(f"mixed call     {t_mixed * 1e3:8.1f} ms, {N} steps: {t_mixed * 1e3 / N:.3f} ms per step")
    if not args.mixed_only:
        def session(timing=None, nreq=B):
            out = {}
            with gen.open_session(nreq, sharp_f=0.0, bright_f=0.0, cond_rows=128) as sess:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                tickets = [sess.admit(labels[b], noise=eps[b], n_iter=N, class_guidance=6, exponent=1) for b in range(nreq)]
                torch.cuda.synchronize(); t1 = time.perf_counter()
                host = 0.0
                for _ in range(N):
                    h0 = time.perf_counter(); out.update(sess.step()); host += time.perf_counter() - h0
                torch.cuda.synchronize(); t2 = time.perf_counter()
                if timing is not None:
                    timing.append((t1 - t0, t2 - t1, host))
            return torch.stack([out[t] for t in tickets])

        got = session(); torch.cuda.synchronize()
        tm = []
        for _ in range(args.iters):
            session(tm)
        t_admit, t_steps, t_host = (median([v[k] for v in tm]) for k in range(3))
        res["session"] = {"ms_steps": round(t_steps * 1e3, 2), "ms_per_step": round(t_steps * 1e3 / N, 3), "ms_admit_64": round(t_admit * 1e3, 2),
                          "ms_total": round((t_admit + t_steps) * 1e3, 2), "host_ms_per_step_call": round(t_host * 1e3 / N, 3),
                          "ms_steps_all": [round(v[1] * 1e3, 2) for v in tm], "classes_ms": class_times(m, session)}
        res["session_bitwise_equal_mixed"] = bool(torch.equal(got, want))
        res["session_step_over_mixed_step"] = round(t_steps / t_mixed, 4)
        res["session_total_over_mixed"] = round((t_admit + t_steps) / t_mixed, 4)
        print(f"session        {t_steps * 1e3:8.1f} ms for {N} steps: {t_steps * 1e3 / N:.3f} ms per step ({t_host * 1e3 / N:.3f} ms of it inside the step call on the host); "
              f"64 admissions {t_admit * 1e3:.1f} ms; steps / mixed call {t_steps / t_mixed:.3f} x, total / mixed call {(t_admit + t_steps) / t_mixed:.3f} x; "
              f"bitwise equal: {res['session_bitwise_equal_mixed']}")
        # one request alone: the chip is almost empty, so the host's share of a step shows
        def one():
            return gen.generate_latents_requests(labels[:1], n_iter=N, class_guidance=6, seeds=eps[:1], **kw)

        one(); session(nreq=1); torch.cuda.synchronize()
        ts, tm = [], []
        for _ in range(args.iters):
            t0 = time.perf_counter(); one(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t0)
            session(tm, nreq=1)
        res["one_request"] = {"mixed_call_ms": round(median(ts) * 1e3, 2), "session_steps_ms": round(median([v[1] for v in tm]) * 1e3, 2),
                              "session_admit_ms": round(median([v[0] for v in tm]) * 1e3, 2),
                              "session_host_ms_per_step_call": round(median([v[2] for v in tm]) * 1e3 / N, 3)}
        print(f"one request    mixed call {res['one_request']['mixed_call_ms']:.2f} ms; session {res['one_request']['session_steps_ms']:.2f} ms for {N} steps + "
              f"{res['one_request']['session_admit_ms']:.2f} ms admission, {res['one_request']['session_host_ms_per_step_call']:.3f} ms per step call on the host")
        for c in _lib.KERNEL_CLASSES:
            print(f"    {c:14s} mixed {res['mixed_call']['classes_ms'][c]:9.3f} ms   session {res['session']['classes_ms'][c]:9.3f} ms")
    m._drop_engine()

if args.leg in ("trace", "both") and not args.mixed_only:
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, ContinuousBatcher, DiffusionTransformer, LTDConfig, RequestBatcher, VaeDecoderConfig
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(dev)
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2, max_batch=args.slots).to(dev)

    class Tok:                               # clip.tokenize stand-in: SOT, one id per character, EOT, zero padding
        def tokenize(self, prompts, truncate=True):
            t = torch.zeros(len(prompts), ccfg.context_length, dtype=torch.long)
            for i, p in enumerate(prompts):
                ids = [1 + (ord(ch) % 900) for ch in p][: ccfg.context_length - 2]
                t[i, 0] = ccfg.vocab_size - 2
                t[i, 1:1 + len(ids)] = torch.tensor(ids)
                t[i, 1 + len(ids)] = ccfg.vocab_size - 1
            return t

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=cfg), vae=vae, clip_model=enc, tokenizer=Tok(), run_device=dev)
    pipe.diffuser.model.load_state_dict(sd)
    pipe.diffuser.model.reserve(2 * args.slots, dev)
    rng = np.random.default_rng(args.seed)
    arrive = np.cumsum(rng.integers(0, 6, size=args.requests)).tolist()
    n_iter = rng.choice([10, 15, 20, 25, 35], size=args.requests).tolist()
    trace = list(zip(arrive, n_iter))
    res["trace"] = {"seed": args.seed, "slots": args.slots, "dt_ms": args.dt_ms, "requests": trace}
    at = [a * args.dt_ms * 1e-3 for a in arrive]

    def timed(fn):
        torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def replay(submit, busy, work):
        """The event loop both batchers share: requests are submitted once the clock has reached their arrival; ``work()`` is one step / one flush
        and returns the tickets it finished; an idle batcher skips to the next arrival."""
        clock, k, done_at, ticket_req = 0.0, 0, {}, {}
        while len(done_at) < len(trace):
            while k < len(trace) and at[k] <= clock:
                t, dt = timed(lambda: submit(k))      # (the continuous batcher encodes the text here, the other one inside its flush)
                ticket_req[t] = k
                clock += dt
                k += 1
            if not busy():
                clock = at[k]
                continue
            finished, dt = timed(work)
            clock += dt
            for t in finished:
                done_at[ticket_req[t]] = clock
        lat = np.array([done_at[i] - at[i] for i in range(len(trace))]) * 1e3
        return {"latency_ms_mean": round(float(lat.mean()), 2), "latency_ms_p50": round(float(np.percentile(lat, 50)), 2),
                "latency_ms_p95": round(float(np.percentile(lat, 95)), 2), "makespan_ms": round(clock * 1e3, 2)}

    def run_continuous():
        with ContinuousBatcher(pipe, slots=args.slots) as cb:
            out = replay(lambda i: cb.submit(f"prompt {i}", 6.0, 100 + i, n_iter[i]), lambda: cb.pending() or cb.live, lambda: list(cb.step()))
            st = cb.session.stats()
        out["model_sample_rows"] = st["rows_cond"] + st["rows_uncond"]
        out["session_steps"] = st["steps"]
        return out

    def run_flushed():
        rb = RequestBatcher(pipe, max_batch=args.slots, mixed=True)
        rows = [0]
        inner = pipe.diffuser.generate_latents_requests

        def counted(*a, **k):
            r = inner(*a, **k)
            rows[0] += sum(pipe.diffuser.model.sample_rows())
            return r

        pipe.diffuser.generate_latents_requests = counted
        try:
            out = replay(lambda i: rb.submit(f"prompt {i}", 6.0, 100 + i, n_iter[i]), rb.pending, lambda: list(rb.flush()))
        finally:
            del pipe.diffuser.generate_latents_requests
        out["model_sample_rows"] = rows[0]
        return out

    run_continuous(); run_flushed()          # warm: engines, kernels, allocator
    res["trace"]["continuous_batcher"] = run_continuous()
    res["trace"]["request_batcher_mixed_flushed_when_idle"] = run_flushed()
    for name in ("continuous_batcher", "request_batcher_mixed_flushed_when_idle"):
        r = res["trace"][name]
        print(f"{name:42s} latency mean {r['latency_ms_mean']:8.1f} ms, p50 {r['latency_ms_p50']:8.1f}, p95 {r['latency_ms_p95']:8.1f}; makespan {r['makespan_ms']:8.1f} ms; "
              f"{r['model_sample_rows']} model-sample rows")

line = json.dumps(res)
print(line)
if args.json:
    with open(args.json, "w") as f:
        f.write(line + "\n")

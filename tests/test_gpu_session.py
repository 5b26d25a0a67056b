"""GPU: sampler sessions (tld_session_*) -- requests admitted between the steps of a running batch.

The defining rule is bitwise: whatever slot a request sits in, whichever step it was admitted at and whoever runs beside it, its end latent is
what ``generate_latents_requests`` returns for that request alone (B = 1, the same arguments).  Every equality here is ``torch.equal``."""
from dataclasses import asdict

import numpy as np
import pytest
import torch

from conftest import cfg_from_arr, load_golden, synth_weights

pytestmark = pytest.mark.gpu

_CACHE = {}
TINY, BIG = "g2_tiny32_sampler.npz", "g5_100m.npz"

# the requests of tests/test_gpu_requests.py
FIVE = dict(class_guidance=[1.0, 3.0, 4.5, 6.0, 3.0], n_iter=[8, 5, 8, 3, 5], use_ddpm_plus=[True, True, False, True, True], exponent=[1, 1, 1, 1, 2])
BIG3 = dict(class_guidance=[6.0, 3.0, 4.5], n_iter=[4, 6, 6], use_ddpm_plus=[True, True, False], exponent=[1, 1, 2])


def _dev():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _model(fixture, low_latency=0):
    key = (fixture, low_latency)
    if key not in _CACHE:
        from transformer_latent_diffusion_amd import Denoiser, DiffusionGenerator
        g = load_golden(fixture)
        cfg = cfg_from_arr(g["cfg"])
        sd = synth_weights(cfg, g["weight_seed"], g["weight_checksum"])
        m = Denoiser(**asdict(cfg)).to(_dev())
        if low_latency:
            m.set_low_latency(low_latency)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
        _CACHE[key] = (m, DiffusionGenerator(m, None, _dev(), torch.float32))
    return _CACHE[key]


def _inputs(B, S=32, seed=61):
    gen = torch.Generator().manual_seed(seed)
    eps = torch.randn(B, 4, S, S, generator=gen)
    labels = torch.randn(B, 768, generator=gen) * 0.5
    negs = torch.randn(B, 768, generator=gen) * 0.5
    return eps, labels, negs


def _requests(kw, B, **extra):
    """One dict of per-request scalars per request, from the per-key lists of FIVE / BIG3 (and of ``extra``)."""
    out = [{k: v[b] for k, v in kw.items()} for b in range(B)]
    for k, v in extra.items():
        for b in range(B):
            if v[b] is not None:
                out[b][k] = v[b]
    return out


def _solo(gen, eps, labels, b, rq, sharp=0.1, bright=0.1):
    """Request b alone through generate_latents_requests with B = 1: (latent [C,S,S], (cond, uncond) model samples of that call)."""
    kw = dict(rq)
    neg = kw.pop("negative_label", None)
    noise_seed = kw.pop("noise_seed", None)
    if "guidance_schedule" in kw:
        kw["guidance_schedule"] = [kw["guidance_schedule"]]
    if noise_seed is not None:
        kw["noise_seeds"] = [noise_seed]
    lat = gen.generate_latents_requests(labels[b:b + 1], seeds=eps[b:b + 1], img_size=32, sharp_f=sharp, bright_f=bright,
                                        negative_labels=None if neg is None else [neg], **kw)
    return lat[0], gen.model.sample_rows()


def _run(gen, slots, eps, labels, reqs, arrivals, sharp=0.1, bright=0.1, cond_rows=None, max_steps=200):
    """The requests through a session of ``slots`` slots; request b is offered before step arrivals[b] and at every later step until it is taken,
    in index order.  Returns (latents by request, log): the slot of each request, how many offers were deferred, the session's final stats."""
    out, slot_of, deferred = {}, {}, 0
    with gen.open_session(slots, sharp_f=sharp, bright_f=bright, cond_rows=cond_rows) as sess:
        ticket_of, waiting, step = {}, list(range(len(reqs))), 0
        while waiting or sess.live:
            assert step < max_steps
            for b in list(waiting):
                if arrivals[b] > step:
                    continue
                t = sess.admit(labels[b], noise=eps[b], **reqs[b])
                if t is None:
                    deferred += 1
                    break                     # (in order: a later request does not overtake)
                ticket_of[t] = b
                slot_of[b] = [s for s, tk in sess._ticket_of.items() if tk == t][0]
                waiting.remove(b)
            for t, lat in sess.step().items():
                out[ticket_of[t]] = lat
            step += 1
        stats = sess.stats()
    return out, dict(slot_of=slot_of, deferred=deferred, stats=stats, steps=step)


def _hold(gen, slots, eps, labels, reqs, arrivals, tag, **kw):
    gen.model.reserve(2 * slots, _dev())      # one engine for the solo calls and the session
    want = [_solo(gen, eps, labels, b, reqs[b], kw.get("sharp", 0.1), kw.get("bright", 0.1)) for b in range(len(reqs))]
    got, log = _run(gen, slots, eps, labels, reqs, arrivals, **kw)
    assert sorted(got) == list(range(len(reqs)))
    for b in range(len(reqs)):
        assert torch.isfinite(got[b]).all()
        assert torch.equal(got[b], want[b][0]), f"{tag}: request {b} (slot {log['slot_of'][b]}) differs from the request alone"
    print(f"{tag}: {len(reqs)} requests in {slots} slots, {log['steps']} steps, slots {log['slot_of']}, {log['deferred']} deferred offers: every end latent "
          f"bitwise equal to the solo call; model samples {log['stats']['rows_cond']} + {log['stats']['rows_uncond']}")
    return got, want, log


# ---- 1. staggered admission, tiny ----------------------------------------------------------------------------------------------------------------------
def test_staggered_admission_tiny():
    m, gen = _model(TINY)
    eps, labels, _ = _inputs(5)
    got, want, log = _hold(gen, 3, eps, labels, _requests(FIVE, 5), [0, 0, 2, 3, 3], "tiny staggered")
    slots = list(log["slot_of"].values())
    assert len(set(slots)) < len(slots), "no slot was reused"
    assert log["deferred"] >= 1, "no admission was deferred"
    assert log["stats"]["live"] == 0 and log["stats"]["cond_rows_used"] == 1


# ---- 2. the 100 M width --------------------------------------------------------------------------------------------------------------------------------
def test_100m_width_changing_live_set():
    """d = 768 at 256 tokens: the fused QKV + attention, the LayerNorm folds and layer-0 sharing, with the third request admitted mid-trajectory."""
    m, gen = _model(BIG)
    eps, labels, _ = _inputs(3, seed=62)
    got, want, log = _hold(gen, 2, eps, labels, _requests(BIG3, 3), [0, 0, 2], "100m")
    assert log["deferred"] >= 1 and log["slot_of"][2] == log["slot_of"][0]


def test_100m_width_low_latency_class_1():
    m, gen = _model(BIG, low_latency=1)
    eps, labels, _ = _inputs(2, seed=63)
    _hold(gen, 2, eps, labels, _requests({k: v[:2] for k, v in BIG3.items()}, 2), [0, 2], "100m low-latency class 1")


# ---- 3. guidance tables and negatives --------------------------------------------------------------------------------------------------------------------
def test_guidance_tables_negatives_and_row_counts():
    """Tables with runs of exactly 1.0: the number of unconditional samples changes from step to step and is 0 at the first two (both live
    requests unguided there).  One request has a negative label.  The session's model-sample counts are the sum of the solo calls'."""
    m, gen = _model(TINY)
    eps, labels, negs = _inputs(3, seed=64)
    f = np.float32
    reqs = [dict(n_iter=5, class_guidance=3.0, guidance_schedule=np.array([1, 1, 3, 3, 1], f)),
            dict(n_iter=4, class_guidance=2.0, guidance_schedule=np.array([1, 1, 1, 2], f), negative_label=negs[1]),
            dict(n_iter=6, class_guidance=4.5, guidance_interval=(0.3, 0.8), use_ddpm_plus=False)]
    got, want, log = _hold(gen, 3, eps, labels, reqs, [0, 0, 2], "guidance tables")
    cond, unc = sum(w[1][0] for w in want), sum(w[1][1] for w in want)
    assert (log["stats"]["rows_cond"], log["stats"]["rows_uncond"]) == (cond, unc), (log["stats"], cond, unc)
    assert cond == 15 and unc < cond
    # the negative label matters, and the first two steps ran no unconditional sample: a session of these two alone counts 9 + 3
    alone = gen.generate_latents_requests(labels[1:2], seeds=eps[1:2], img_size=32, n_iter=4, class_guidance=2.0, guidance_schedule=[reqs[1]["guidance_schedule"]])
    assert not torch.equal(alone[0], got[1])
    got2, log2 = _run(gen, 2, eps, labels, reqs[:2], [0, 0])
    assert (log2["stats"]["rows_cond"], log2["stats"]["rows_uncond"]) == (9, 3) and torch.equal(got2[0], got[0]) and torch.equal(got2[1], got[1])


# ---- 4. stochastic ---------------------------------------------------------------------------------------------------------------------------------------
def test_stochastic_request_admitted_at_step_3():
    """eta = 1 beside deterministic co-tenants, admitted at session step 3: its noise counter must run on its OWN forward index."""
    m, gen = _model(TINY)
    eps, labels, _ = _inputs(3, seed=65)
    reqs = [dict(n_iter=8, class_guidance=3.0), dict(n_iter=6, class_guidance=4.5, use_ddpm_plus=False),
            dict(n_iter=5, class_guidance=3.0, eta=1.0, noise_seed=0x0123456789ABCDEF)]
    got, want, log = _hold(gen, 3, eps, labels, reqs, [0, 0, 3], "stochastic")
    det = gen.generate_latents_requests(labels[2:3], seeds=eps[2:3], img_size=32, n_iter=5, class_guidance=3.0)[0]
    assert not torch.equal(det, got[2]), "the noise changed nothing"
    # all-zero coefficients: bitwise the deterministic request (through the raw session, which takes the table itself)
    from transformer_latent_diffusion_amd import schedule
    co = schedule.step_coefficients(schedule.noise_schedule(5, 1), True)
    with m.open_session(2, sharp_f=0.1, bright_f=0.1) as raw:
        a = raw.admit(eps[2].to(_dev()), labels[2].to(_dev()), co, 3.0, noise_coeff=np.zeros(5, np.float32), noise_key=77)
        b = raw.admit(eps[0].to(_dev()), labels[0].to(_dev()), schedule.step_coefficients(schedule.noise_schedule(8, 1), True), 3.0)
        assert (a, b) == (0, 1)
        done = []
        for _ in range(5):
            done += raw.step()
        assert done == [0]
        assert torch.equal(raw.latent(0), det)


# ---- 5. slot hygiene -------------------------------------------------------------------------------------------------------------------------------------
def test_slot_reuse_leaks_nothing_and_a_finished_latent_stays():
    m, gen = _model(TINY)
    eps, labels, _ = _inputs(2, seed=66)
    reqs = [dict(n_iter=8, class_guidance=3.0), dict(n_iter=3, class_guidance=6.0)]
    # one slot: the long request finishes in slot 0, the short one follows it there (x0_prev of the long one must not reach it)
    got, want, log = _hold(gen, 1, eps, labels, reqs, [0, 0], "one slot")
    assert log["slot_of"] == {0: 0, 1: 0} and log["steps"] == 11
    # two slots: the short request finishes first; its latent, read again after further steps and before the slot is reused, has not moved
    with gen.open_session(2) as sess:
        t_long = sess.admit(labels[0], noise=eps[0], **reqs[0])
        t_short = sess.admit(labels[1], noise=eps[1], **reqs[1])
        slot_short = [s for s, t in sess._ticket_of.items() if t == t_short][0]
        first = {}
        for _ in range(3):
            first.update(sess.step())
        assert list(first) == [t_short] and torch.equal(first[t_short], want[1][0])
        for _ in range(3):
            assert sess.step() == {}
        assert torch.equal(sess.raw.latent(slot_short), want[1][0]), "a finished latent changed before its slot was reused"
        rest = {}
        while sess.live:
            rest.update(sess.step())
        assert torch.equal(rest[t_long], want[0][0])


# ---- 6. order independence -------------------------------------------------------------------------------------------------------------------------------
def test_order_independence():
    m, gen = _model(TINY)
    eps, labels, _ = _inputs(5)
    reqs = _requests(FIVE, 5)
    m.reserve(10, _dev())
    a, _ = _run(gen, 3, eps, labels, reqs, [0, 0, 2, 3, 3])
    b, _ = _run(gen, 5, eps, labels, reqs, [4, 1, 0, 0, 2])
    c, _ = _run(gen, 2, eps, labels, reqs, [0] * 5)
    for k in range(5):
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), f"request {k} depends on the admission timing or the slot count"


# ---- 7. engine state -------------------------------------------------------------------------------------------------------------------------------------
def test_engine_state_around_a_session():
    import ctypes as C
    from transformer_latent_diffusion_amd import _lib
    m, gen = _model(TINY)
    eps, labels, _ = _inputs(2, seed=67)
    call = lambda: gen.generate_latents(labels, n_iter=4, num_imgs=2, class_guidance=3.0, seeds=eps, img_size=32)
    m.reserve(8, _dev())
    before = call()
    fwd = lambda: m(eps.to(_dev()), torch.full((2, 1), 0.5, device=_dev()), labels.to(_dev()))
    fwd_before = fwd()
    with gen.open_session(2) as sess:
        # an empty session: a step launches nothing and returns no ticket
        assert sess.step() == {} and sess.stats() == dict(live=0, steps=0, rows_cond=0, rows_uncond=0, cond_rows_used=1)
        for what, fn in (("generate_latents", call), ("forward", fwd),
                         ("generate_latents_requests", lambda: gen.generate_latents_requests(labels, seeds=eps, img_size=32, n_iter=[4, 3])),
                         ("load_flat", lambda: m.load_flat(torch.zeros(m.param_count)))):
            with pytest.raises(RuntimeError, match=r"status 4.*session is open"):
                fn()
        with pytest.raises(RuntimeError, match="already open"):
            gen.open_session(2)
        with pytest.raises(RuntimeError, match="would destroy it"):
            gen.generate_latents(labels.repeat(20, 1), n_iter=4, num_imgs=40, class_guidance=3.0, seeds=eps.repeat(20, 1, 1, 1), img_size=32)
        # what a session does not take is refused by name
        for kw, text in ((dict(init_latents=eps[0]), "init_latents"), (dict(strength=0.5), "start_mix"), (dict(mask=eps[0, :1]), "mask"),
                         (dict(guidance_rescale=0.5), "guidance shape"), (dict(apg_eta=0.0), "guidance shape"), (dict(trace=True), "trace")):
            with pytest.raises(ValueError, match=text):
                sess.admit(labels[0], noise=eps[0], n_iter=4, **kw)
        # another stream than the session's: refused (TLD_ERR_INVALID); a capturing stream: refused (TLD_ERR_STATE); nothing was admitted or run
        other = torch.cuda.Stream(_dev())
        with torch.cuda.stream(other):
            with pytest.raises(RuntimeError, match=r"status 1.*stream"):
                sess.admit(labels[0], noise=eps[0], n_iter=4)
            with pytest.raises(RuntimeError, match=r"status 1.*stream"):
                sess.step()
        assert sess.stats()["live"] == 0
        t = sess.admit(labels[0], noise=eps[0], n_iter=4, class_guidance=3.0)
        done = {}
        while sess.live:
            done.update(sess.step())
    solo = gen.generate_latents_requests(labels[:1], seeds=eps[:1], img_size=32, n_iter=4, class_guidance=3.0)[0]
    assert torch.equal(done[t], solo)
    # after close: the bits the engine returned before the session
    assert torch.equal(call(), before) and torch.equal(fwd(), fwd_before)
    # a session on a stream of its own; while that stream is capturing a step is refused (TLD_ERR_STATE) and runs nothing, and so is an open
    side = torch.cuda.Stream(_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        with gen.open_session(2) as sess:
            t = sess.admit(labels[0], noise=eps[0], n_iter=4, class_guidance=3.0)
            lab1, eps1 = labels[1].to(_dev()), eps[1].to(_dev())        # (on the device already: the refused admit below copies nothing)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            graph.capture_begin(capture_error_mode="relaxed")
            try:
                with pytest.raises(RuntimeError, match=r"status 4.*captured"):
                    sess.step()
                with pytest.raises(RuntimeError, match=r"status 4.*captured"):
                    sess.admit(lab1, noise=eps1, n_iter=4)
            finally:
                graph.capture_end()
            assert sess.stats()["steps"] == 0 and sess.live == 1
            done = {}
            while sess.live:
                done.update(sess.step())
            side.synchronize()
            assert torch.equal(done[t], solo)
        graph = torch.cuda.CUDAGraph()
        graph.capture_begin(capture_error_mode="relaxed")
        try:
            with pytest.raises(RuntimeError, match=r"status 4.*captured"):
                gen.open_session(2)
        finally:
            graph.capture_end()
    torch.cuda.synchronize()
    assert m._session is None
    L = _lib.lib()
    cfgd = m._cfg
    cfg = _lib.TldConfig(cfgd["image_size"], cfgd["noise_embed_dims"], cfgd["patch_size"], cfgd["embed_dim"], cfgd["n_layers"], cfgd["text_emb_size"],
                         cfgd["n_channels"], cfgd["mlp_multiplier"], 8, 0)
    h, out = C.c_void_p(), C.c_void_p()
    _lib.check(L.tld_engine_create(C.byref(cfg), C.byref(h)), "tld_engine_create")
    try:
        assert L.tld_session_open(h, 2, 8, 0.0, 0.0, None, C.byref(out)) == 4 and L.tld_last_error().decode() == "weights not finalized"
    finally:
        L.tld_engine_destroy(h)
    # the launch path of a session step, under the debug hook: recorded, and no stage kept
    m.set_debug(True)
    try:
        with gen.open_session(2) as sess:
            sess.admit(labels[0], noise=eps[0], n_iter=3)
            sess.step()
            assert m.debug_paths() >> 62 & 1 and not m.debug_paths() >> 58 & 1
            with pytest.raises(RuntimeError):
                m.read_stage("step.x_t")
    finally:
        m.set_debug(False)


# ---- 8. the pipeline -------------------------------------------------------------------------------------------------------------------------------------
def test_continuous_batcher_over_the_native_pipeline():
    from PIL import Image
    from transformer_latent_diffusion_amd import AutoencoderKLDecoder, ContinuousBatcher, DenoiserConfig, DiffusionTransformer, LTDConfig, VaeDecoderConfig
    from transformer_latent_diffusion_amd.clip_text import ClipTextConfig, ClipTextEncoder
    ccfg = ClipTextConfig(vocab_size=1000, context_length=16, width=128, heads=2, layers=2, embed_dim=768)
    enc = ClipTextEncoder(ccfg, init_seed=1).to(_dev())
    vae = AutoencoderKLDecoder(VaeDecoderConfig(block_out_channels=(64, 128), layers_per_block=1), init_seed=2).to(_dev())

    class Tok:                               # clip.tokenize stand-in: SOT, one id per character, EOT, zero padding
        def tokenize(self, prompts, truncate=True):
            t = torch.zeros(len(prompts), ccfg.context_length, dtype=torch.long)
            for i, p in enumerate(prompts):
                ids = [1 + (ord(ch) % 900) for ch in p][: ccfg.context_length - 2]
                t[i, 0] = ccfg.vocab_size - 2
                t[i, 1:1 + len(ids)] = torch.tensor(ids)
                t[i, 1 + len(ids)] = ccfg.vocab_size - 1
            return t

    pipe = DiffusionTransformer(LTDConfig(denoiser_cfg=DenoiserConfig(n_channels=4)), vae=vae, clip_model=enc, tokenizer=Tok(), run_device=_dev())
    prompts, guid, n_it, seeds = ["a cute cat", "a red car", "a tall tree", "a cute cat"], [6.0, 3.0, 4.5, 6.0], [4, 6, 4, 5], [3, 4, 5, 6]
    extra = [dict(), dict(negative_prompt="blurry"), dict(guidance_interval=(0.3, 0.8)), dict(eta=1.0)]                     # what submit takes ...
    extra_alone = [dict(), dict(negative_prompts=["blurry"]), dict(guidance_interval=(0.3, 0.8)), dict(eta=[1.0])]            # ... and the one-prompt call
    pipe.diffuser.model.reserve(8, _dev())
    alone, alone_lat = [], []
    inner = pipe.diffuser._decode
    pipe.diffuser._decode = lambda lat, sf: (alone_lat.append(lat.clone()), inner(lat, sf))[1]
    try:
        for i in range(4):
            alone.append(pipe.generate_images_from_texts([prompts[i]], class_guidance=guid[i], seeds=[seeds[i]], n_iter=n_it[i], **extra_alone[i])[0])
    finally:
        del pipe.diffuser._decode
    assert len(alone_lat) == 4
    got_lat = {}
    with ContinuousBatcher(pipe, slots=2) as cb:
        orig = cb.session.step
        cb.session.step = lambda: (lambda d: (got_lat.update(d), d)[1])(orig())
        with pytest.raises(ValueError, match="guidance shape"):
            cb.submit("x", guidance_rescale=0.5)
        tickets, pics = [], {}
        tickets.append(cb.submit(prompts[0], guid[0], seeds[0], n_it[0], **extra[0]))
        tickets.append(cb.submit(prompts[1], guid[1], seeds[1], n_it[1], **extra[1]))
        pics.update(cb.step())
        pics.update(cb.step())
        tickets.append(cb.submit(prompts[2], guid[2], seeds[2], n_it[2], **extra[2]))       # waits for a slot
        pics.update(cb.step())
        tickets.append(cb.submit(prompts[3], guid[3], seeds[3], n_it[3], **extra[3]))
        assert cb.pending() == 2 and cb.live == 2
        pics.update(cb.drain())
        assert cb.pending() == 0 and cb.live == 0
    assert sorted(pics) == tickets and all(isinstance(p, Image.Image) for p in pics.values())
    session_tickets = sorted(got_lat)
    for i, t in enumerate(tickets):
        assert torch.equal(got_lat[session_tickets[i]], alone_lat[i][0]), f"prompt {i}: the session's latent differs from the one-prompt call's"
        assert np.array_equal(np.asarray(pics[t]), np.asarray(alone[i])), f"prompt {i}: the picture differs from the one-prompt call's"

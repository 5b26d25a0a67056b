"""Training step of the denoiser on the gfx950 engine -- the host side of ``tld_train_*``.

Mirrors the body of the reference's training loop (tld/train.py:118-175) for one batch:

    noise_level ~ Beta(beta_a, beta_b);  x_noisy = noise_level * noise + (1 - noise_level) * x       (:120-130)  -> make_batch / mix_noise
    label[rand < 0.15] = 0                                                                           (:135-138)  -> make_batch / drop_labels
    pred = model(x_noisy, noise_level.view(-1, 1), label); loss = MSELoss(pred, x); backward         (:160-168)  -> Trainer.forward_backward
    gradient all-reduce of accelerate's DDP wrapper                                                  (:114,168)  -> Trainer.optimizer_step (RCCL)
    optimizer.step()  (Adam, lr) ; update_ema(ema_model, model, alpha)                               (:87,169-172,55-58) -> Trainer.optimizer_step

Parameters, gradients, Adam moments and the EMA copy are flat fp32 torch tensors on the device (PyTorch owns the memory and the
collective; the arithmetic is in libtld_hip.so).  There is no CPU path: constructing a ``Trainer`` without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
from collections import OrderedDict
from dataclasses import asdict, dataclass
from typing import Dict, Mapping, Optional, Tuple

import numpy as np
import torch

from . import _lib, opt_groups
from .configs import DenoiserConfig
from .weights import param_layout, state_dict_spec, synth_state_dict, unflatten  # noqa: F401  (param_layout: this module's name for it stays)

LABEL_DROPOUT = 0.15                 # tld/train.py:135


@dataclass
class TrainConfig:
    """tld/configs.py:58-72 (the fields the step itself reads: lr, alpha, beta_a, beta_b, batch_size)."""
    batch_size: int = 128
    lr: float = 3e-4
    n_epoch: int = 100
    alpha: float = 0.999
    from_scratch: bool = True
    beta_a: float = 1
    beta_b: float = 2.5
    save_and_eval_every_iters: int = 1000
    run_id: str = ""
    model_name: str = ""
    compile: bool = True
    save_model: bool = True
    use_wandb: bool = True


def mix_noise(x: torch.Tensor, noise_level: torch.Tensor, noise: torch.Tensor) -> torch.Tensor:
    """tld/train.py:123-130: ``noise_level`` is float64 there (np.random.beta), so the mix is formed in float64 and cast to float32."""
    nl = noise_level.to(torch.float64).view(-1, 1, 1, 1)
    return (nl * noise + (1 - nl) * x).float()


def drop_labels(y: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """tld/train.py:135-138 (on a copy: the reference mutates the batch tensor the loader yields)."""
    out = y.clone()
    out[mask] = 0
    return out


def allreduce_mean_(flat: torch.Tensor, group=None) -> float:
    """DDP's gradient averaging as one collective on the flat vector: SUM all-reduce in place; returns the factor (1 / world size)
    the optimizer kernel applies (tld/train.py:114,168: accelerate's DDP wrapper).  No-op without an initialised process group."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        return 1.0 / dist.get_world_size(group)
    return 1.0


def update_ema_(ema: torch.Tensor, params: torch.Tensor, alpha: float = 0.999) -> None:
    """tld/train.py:55-58 on flat vectors (host-side statement of what the fused kernel does; used by tests)."""
    ema.mul_(alpha).add_(params, alpha=1 - alpha)


EVAL_SEED_XOR = 0x5851F42D4C957F2D     # eval_loss's default Philox key is data_seed ^ this: the evaluation never meets the training stream


def bucket_midpoints(n_buckets: int) -> np.ndarray:
    """The default evaluation levels: the midpoints (k + 0.5) / n of the n noise-level bins, float64."""
    return (np.arange(int(n_buckets), dtype=np.float64) + 0.5) / float(n_buckets)


def eval_plan(n: int, batch_size: int, world: int, rank: int, levels):
    """The batch / level plan of ``Trainer.eval_loss``, a pure host function: the ``n`` positions of the evaluation are cut into batches
    ``[j * batch_size, (j + 1) * batch_size)`` (the last one may be short), rank ``r`` of ``world`` takes the batches ``j = r (mod world)``, and
    global position ``p`` is evaluated at ``levels[p % len(levels)]`` whatever the world size.  Returns ``[(j, start, stop, levels float64
    [stop - start]), ...]`` for this rank, in the order it runs them."""
    n, batch_size, world, rank = int(n), int(batch_size), int(world), int(rank)
    lv = np.asarray(levels, dtype=np.float64).reshape(-1)
    if n < 0 or batch_size < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"eval_plan(n={n}, batch_size={batch_size}, world={world}, rank={rank})")
    if lv.size == 0 or not bool(np.all((lv >= 0.0) & (lv <= 1.0))):          # (NaN fails the comparison)
        raise ValueError("noise levels must be a non-empty sequence inside [0, 1]")
    plan = []
    for j in range(rank, (n + batch_size - 1) // batch_size, world):
        start, stop = j * batch_size, min(n, (j + 1) * batch_size)
        plan.append((j, start, stop, lv[np.arange(start, stop) % lv.size]))
    return plan


class EvalLoss:
    """Loss by noise level: the device state vector of ``tld_train_loss_buckets`` (fp64 ``[2 n + 2]``: sums per bucket, counts, total sum, rejected
    count) and its readouts.  Every property is a device tensor computed without a host wait; ``cpu()`` synchronises and returns a dict."""

    def __init__(self, n_buckets: int, device=None, state: Optional[torch.Tensor] = None):
        self.n_buckets = int(n_buckets)
        if not 1 <= self.n_buckets <= 256:
            raise ValueError(f"n_buckets = {n_buckets}: 1 .. 256")
        self.state = state if state is not None else torch.zeros(2 * self.n_buckets + 2, dtype=torch.float64, device=device)
        if self.state.dtype != torch.float64 or self.state.numel() != 2 * self.n_buckets + 2:
            raise ValueError("state must be float64 [2 n_buckets + 2]")

    def zero_(self) -> "EvalLoss":
        self.state.zero_()
        return self

    @property
    def bucket_count(self) -> torch.Tensor:
        return self.state[self.n_buckets:2 * self.n_buckets]

    @property
    def bucket_loss(self) -> torch.Tensor:
        """Mean loss per bucket; NaN where the bucket is empty."""
        c = self.bucket_count
        return torch.where(c > 0, self.state[:self.n_buckets] / c, torch.full_like(c, float("nan")))

    @property
    def loss(self) -> torch.Tensor:
        """Mean loss over every accepted sample (NaN when there is none)."""
        return self.state[2 * self.n_buckets] / self.bucket_count.sum()

    @property
    def rejected(self) -> torch.Tensor:
        return self.state[2 * self.n_buckets + 1]

    def cpu(self) -> Dict[str, object]:
        st = self.state.detach().cpu().numpy()
        n = self.n_buckets
        cnt = st[n:2 * n]
        with np.errstate(invalid="ignore", divide="ignore"):
            return {"loss": float(st[2 * n] / cnt.sum()) if cnt.sum() > 0 else float("nan"),
                    "bucket_loss": np.where(cnt > 0, st[:n] / np.where(cnt > 0, cnt, 1.0), np.nan), "bucket_count": cnt.astype(np.int64),
                    "rejected": int(st[2 * n + 1]), "n_buckets": n}


class Trainer:
    """One model replica + optimizer state on one device.  With ``torch.distributed`` initialised (backend ``nccl`` = RCCL) every rank
    holds a replica, gradients are summed with one all-reduce of the flat vector per step and divided by the world size."""

    def __init__(self, denoiser_cfg: DenoiserConfig, train_cfg: Optional[TrainConfig] = None, device="cuda",
                 state_dict: Optional[Mapping[str, torch.Tensor]] = None, init_seed: int = 0, max_batch: Optional[int] = None,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, keep_ema: bool = True, process_group=None,
                 overlap_allreduce: bool = True, use_graph: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, data_seed: int = 0, loss_buckets: Optional[int] = None, weight_decay: float = 0.0,
                 param_groups=None, lr_schedule=None, schedule_steps: Optional[int] = None):
        self.cfg = denoiser_cfg
        self.tc = train_cfg if train_cfg is not None else TrainConfig()
        dev = torch.device(device)
        if dev.type != "cuda" or not torch.cuda.is_available():
            raise RuntimeError("Trainer needs a HIP device ('cuda'); the training engine has no CPU path")
        # ONE device for the engine, the flat tensors and the stream: "cuda" means the caller's CURRENT device (torch.cuda.set_device(local_rank)
        # under torch.distributed.run), exactly as Denoiser resolves it -- not device 0
        self.device = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        if float(denoiser_cfg.dropout) != 0.0:
            # the reference trains with model.train(): dropout_p in SDPA and nn.Dropout in the MLP (tld/transformer_blocks.py:43,105).  The engine's
            # training forward has no dropout; training a different model silently is worse than refusing (every published config has dropout = 0)
            raise NotImplementedError(f"DenoiserConfig.dropout = {denoiser_cfg.dropout}: the training engine implements dropout = 0 only")
        self.betas, self.eps = betas, eps
        if max_grad_norm is not None and np.isnan(float(max_grad_norm)):
            raise ValueError("max_grad_norm is NaN")
        # the guarded optimizer step (optimizer_step): either option makes the trainer own the guard's fp64 device state vector
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        self.guarded = self.max_grad_norm is not None or self.skip_nonfinite
        self._opt_state = None
        self.group = process_group
        self.layout = param_layout(denoiser_cfg)
        # the grouped optimizer step (opt_groups): any of weight_decay / param_groups / lr_schedule makes the trainer own a
        # tld_opt_plan and the fp64 state; with all three at their defaults nothing is built and the three step paths below run as they always did
        self.weight_decay = float(weight_decay)
        self.grouped = self.weight_decay != 0.0 or bool(param_groups) or lr_schedule is not None
        self._plan = None
        self._lr_table = None
        if self.grouped:
            self._seg_numel, self._seg_group, self._groups = opt_groups.resolve(self.layout, param_groups, self.weight_decay)
            if lr_schedule is not None:
                self._lr_table = opt_groups.lr_table(lr_schedule, schedule_steps)
        self.numel = sum(int(np.prod(s)) for _, s in self.layout.values())
        c = asdict(denoiser_cfg)
        L = _lib.lib()
        self.max_batch = int(max_batch if max_batch is not None else self.tc.batch_size)
        cc = _lib.TldConfig(c["image_size"], c["noise_embed_dims"], c["patch_size"], c["embed_dim"], c["n_layers"], c["text_emb_size"],
                            c["n_channels"], c["mlp_multiplier"], self.max_batch, self.device.index)
        h = C.c_void_p()
        _lib.check(L.tld_train_create(C.byref(cc), C.byref(h)), "tld_train_create")
        self._h = h
        try:
            self._check_layout()
            z = lambda: torch.zeros(self.numel, dtype=torch.float32, device=self.device)
            self.params, self.grads, self.exp_avg, self.exp_avg_sq = z(), z(), z(), z()
            self.ema = z() if keep_ema else None
            self.step = 0
            if self.grouped:
                self._build_plan()
            if self.guarded or self.grouped:              # all zeros = a fresh optimizer (include/tld_hip.h); a step allocates nothing
                self._opt_state = torch.zeros(_lib.TRAIN_OPT_STATE_DOUBLES, dtype=torch.float64, device=self.device)
            sd = state_dict if state_dict is not None else {k: torch.from_numpy(np.array(v)) for k, v in synth_state_dict(denoiser_cfg, init_seed).items()}
            self.load_state_dict(sd)
            _lib.check(L.tld_train_bind(self._h, C.c_void_p(self.params.data_ptr()), C.c_void_p(self.grads.data_ptr())), "tld_train_bind")
        except Exception:
            self._destroy_plan()
            L.tld_train_destroy(self._h)
            self._h = None
            raise
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        # HIP-graph replay of forward + backward: the step is ~1 900 small launches with static shapes; captured once (on the second full-batch
        # call, after an eager warm-up) and replayed from fixed input buffers, it takes the host out of the loop.  Adam stays outside (its step
        # count is a kernel argument).  Round 5: ON by default for a single replica (TLD_TRAIN_GRAPH=0 / use_graph=False: eager launches) -- on a
        # slow host the eager step's wall time was 44 ms against 31 ms of device time; with more than one rank the eager path stays the default,
        # because the per-block gradient all-reduces are launched from a host callback in the middle of the backward (not capturable).
        # precedence: the explicit constructor argument, then TLD_TRAIN_GRAPH, then the default (one replica: on).  The world size is read
        # here; a process group initialised later does not flip the choice, so a graph step with more than one rank (which gives up the
        # overlapped per-block all-reduce for full batches) is announced once, at the first such step (forward_backward).
        env = os.environ.get("TLD_TRAIN_GRAPH")
        self.use_graph = bool(use_graph) if use_graph is not None else (bool(int(env)) if env is not None else self._world() == 1)
        self._graph_world_warned = False
        self.overlap_allreduce = overlap_allreduce
        self._comm_stream = None
        self._pending = []                # async all-reduce handles of the gradient slices of the step in flight
        self._reduced = False             # True between an overlapped forward_backward and the optimizer_step that consumes its reduced gradients
        self._cb_error = None             # first exception raised inside the gradient-ready callback (ctypes would swallow it)
        self.global_step = 0              # tld/train.py:104,174 -- the loop counter the checkpoint carries; Adam's own count is self.step
        self._slices = []                 # (offset, numel) in the order they became ready (tests)
        self._graph = None
        self._graph_calls = 0
        self._debug = False
        self._static = None
        # gradient accumulation over micro-batches (accelerator.accumulate(), tld/train.py:160)
        self._acc = None                  # flat fp32 sum of the gradients of the micro-batches folded so far
        self._acc_n = 0
        self._micro_scale = 1.0           # 1 / (micro-batches of the step): applied by the optimizer kernel together with 1 / world
        # host -> device staging of train_step's batch: pinned double buffers + a copy stream, so that the host never blocks on a pageable copy
        # that is stream-ordered behind the previous step's kernels (that stall made the eager step's wall time device + enqueue time)
        self._stage = [None, None]
        self._stage_i = 0
        self._copy_stream = None
        self._eval_den = None             # eval_generate's denoiser (built on the first call, synced on every one)
        # the device data path (prepare_batch / train_step_from): the Philox key of every draw, and the kernel's count of refused row indices
        self.data_seed = int(data_seed) & (2 ** 64 - 1)
        self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        # loss by noise level: the batch of the engine's last forward (sample_loss), and with loss_buckets=n the running accumulator of the training loss
        self._last_batch = 0
        self.train_loss_levels = EvalLoss(loss_buckets, self.device) if loss_buckets is not None else None

    def _check_layout(self):
        L = _lib.lib()
        n = L.tld_train_tensor_count(self._h)
        if n != len(self.layout) or L.tld_train_param_count(self._h) != self.numel:
            raise RuntimeError("parameter layout of the engine and of weights.state_dict_spec disagree")
        buf = C.create_string_buffer(256)
        off, num = C.c_int64(), C.c_int64()
        for i, (k, (o, s)) in enumerate(self.layout.items()):
            _lib.check(L.tld_train_param_layout(self._h, i, buf, 256, C.byref(off), C.byref(num)), "tld_train_param_layout")
            if buf.value.decode() != k or off.value != o or num.value != int(np.prod(s)):
                raise RuntimeError(f"parameter layout mismatch at {i}: engine {buf.value.decode()}@{off.value}+{num.value}, host {k}@{o}")

    def _build_plan(self) -> None:
        """``tld_opt_plan_create`` from the resolved groups: the tables go up once, here."""
        n, ng = len(self._seg_numel), len(self._groups)
        numel = (C.c_int64 * n)(*self._seg_numel)
        group = (C.c_int32 * n)(*self._seg_group)
        gs = (_lib.TldOptGroup * ng)(*[_lib.TldOptGroup(s, w, int(f), 0) for s, w, f in self._groups])
        tab = self._lr_table
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_opt_plan_create(self.device.index, numel, group, n, gs, ng,
                                                      tab.ctypes.data_as(C.POINTER(C.c_float)) if tab is not None else None,
                                                      int(tab.size) if tab is not None else 0, C.byref(h)), "tld_opt_plan_create")
        self._plan = h
        if _lib.lib().tld_opt_plan_numel(h) != self.numel:
            raise RuntimeError("the optimizer plan and the parameter layout disagree on the vector's length")
        ptr = C.c_void_p()
        _lib.check(_lib.lib().tld_opt_plan_segment_sqsums(h, C.byref(ptr)), "tld_opt_plan_segment_sqsums")

        class _View:                      # the plan's device double [n_tensors], handed to torch without a copy
            __cuda_array_interface__ = {"shape": (n,), "typestr": "<f8", "data": (int(ptr.value), False), "version": 2, "strides": None}
        with torch.cuda.device(self.device):
            self._seg_sq = torch.as_tensor(_View(), device=self.device)

    def _destroy_plan(self) -> None:
        if getattr(self, "_plan", None) is not None:
            self._seg_sq = None
            _lib.lib().tld_opt_plan_destroy(self._plan)
            self._plan = None

    def __del__(self):
        try:
            self._destroy_plan()
            if getattr(self, "_h", None) is not None:
                _lib.lib().tld_train_destroy(self._h)
                self._h = None
        except Exception:
            pass

    # ---- state ----------------------------------------------------------------------------------------------------------------
    def _unflatten(self, flat: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        return unflatten(flat, self.cfg)

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Views into the live flat parameter vector, reference keys (+ the two registered buffers)."""
        sd = self._unflatten(self.params)
        sd["fourier_feats.0.angular_speeds"] = self._angular
        return sd

    def ema_state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """What the reference saves as ``model_ema`` (tld/train.py:150-156) and the inference ``Denoiser`` loads."""
        if self.ema is None:
            raise RuntimeError("this Trainer keeps no EMA copy (keep_ema=False)")
        sd = OrderedDict((k, v.clone()) for k, v in self._unflatten(self.ema).items())
        sd["fourier_feats.0.angular_speeds"] = self._angular.clone()
        sd["denoiser_trans_block.precomputed_pos_enc"] = torch.arange(self.layout["denoiser_trans_block.pos_embed.weight"][1][0])
        return sd

    def grad_dict(self) -> "OrderedDict[str, torch.Tensor]":
        """Views into the flat gradient vector.  In overlap mode with more than one rank these are the cross-rank SUM (not the mean) once the
        slice reductions have been waited for, which this does."""
        self.wait_gradients()
        return self._unflatten(self.grads)

    def load_state_dict(self, sd: Mapping[str, torch.Tensor]) -> "Trainer":
        missing = [k for k in self.layout if k not in sd]
        if missing:
            raise RuntimeError(f"missing keys in state_dict: {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        host = torch.empty(self.numel, dtype=torch.float32)
        for k, (o, s) in self.layout.items():
            t = (sd[k] if isinstance(sd[k], torch.Tensor) else torch.as_tensor(np.asarray(sd[k]))).detach().to(torch.float32).cpu()
            if tuple(t.shape) != s:
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(t.shape)}, model {s}")
            host[o:o + t.numel()] = t.reshape(-1)
        self.params.copy_(host)
        if self.ema is not None:
            self.ema.copy_(host)                                  # ema_model = copy.deepcopy(model)   (tld/train.py:110-111)
        ang = sd.get("fourier_feats.0.angular_speeds")
        if ang is None:
            ang = torch.from_numpy(np.array(synth_state_dict(self.cfg, 0)["fourier_feats.0.angular_speeds"]))
        self._angular = (ang if isinstance(ang, torch.Tensor) else torch.as_tensor(np.asarray(ang))).detach().to(torch.float32).cpu().contiguous()
        a = self._angular.numpy()
        _lib.check(_lib.lib().tld_train_set_angular_speeds(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), a.size), "tld_train_set_angular_speeds")
        _lib.check(_lib.lib().tld_train_bind(self._h, C.c_void_p(self.params.data_ptr()), C.c_void_p(self.grads.data_ptr())), "tld_train_bind")
        if getattr(self, "_acc_n", 0):
            self.reset_accumulation()                             # gradients folded against the old weights mean nothing for the new ones
        return self

    # ---- stage hook (tests) ---------------------------------------------------------------------------------------------------
    # launch paths reported by debug_paths(), bit number = position (the table in include/tld_hip.h)
    PATH_NAMES = ("resid_ln_q4<1>", "resid_ln_q4<2>", "resid_ln_q4<3>", "resid_ln_q4<4>", "resid_ln_generic", "ln_bwd_q4<1>", "ln_bwd_q4<2>", "ln_bwd_q4<3>",
                  "ln_bwd_generic", "embed_lds<1>", "embed_lds<2>", "embed_lds<3>", "embed_lds<4>", "embed_plain", "tail_dx4<16>", "tail_dx4<32>", "tail_dx4<64>",
                  "tail_dx_generic", "tall_dw_cols", "tall_dw_partial", "colsum4", "colsum", "dw_bwd_fused", "dw_bwd_unfused", "wgrad_tn", "wgrad_transposing_sk1",
                  "wgrad_transposing_splitk", "wgrad_transposing_padded", "attn_bwd_one_kernel", "attn_bwd_two_kernels", "attn_bwd_masked")

    def set_debug(self, enable: bool = True) -> "Trainer":
        """Stage capture (``tld_train_set_debug``): the next ``forward_backward`` calls poison the engine's buffers first, keep every stage for
        ``read_stage`` and record their launch paths; they run eagerly (never through the captured graph).  Off again: snapshots are freed."""
        _lib.check(_lib.lib().tld_train_set_debug(self._h, 1 if enable else 0), "tld_train_set_debug")
        self._debug = bool(enable)
        return self

    debug = property(lambda self: self._debug, lambda self, v: self.set_debug(v) and None)

    def read_stage(self, name: str) -> torch.Tensor:
        """A stage of the last debug step as a float32 host tensor with its logical shape (names: include/tld_hip.h)."""
        L = _lib.lib()
        shape = (C.c_int64 * 4)()
        _lib.check(L.tld_train_read_stage(self._h, name.encode(), None, 0, shape), f"tld_train_read_stage({name})")
        dims = [int(v) for v in shape]
        while len(dims) > 1 and dims[-1] == 1:
            dims.pop()
        out = torch.empty(int(np.prod(dims)), dtype=torch.float32)
        _lib.check(L.tld_train_read_stage(self._h, name.encode(), C.cast(out.data_ptr(), C.POINTER(C.c_float)), out.numel(), shape),
                   f"tld_train_read_stage({name})")
        return out.view(*dims)

    def debug_paths(self) -> int:
        m = C.c_uint64()
        _lib.check(_lib.lib().tld_train_debug_paths(self._h, C.byref(m)), "tld_train_debug_paths")
        return int(m.value)

    # ---- the step -------------------------------------------------------------------------------------------------------------
    def make_batch(self, x: torch.Tensor, y: torch.Tensor, np_rng: Optional[np.random.Generator] = None,
                   generator: Optional[torch.Generator] = None):
        """tld/train.py:118-138 for one (latents, text embeddings) batch: returns (x_noisy, noise_level fp32, label)."""
        rng = np_rng if np_rng is not None else np.random.default_rng()
        noise_level = torch.tensor(rng.beta(self.tc.beta_a, self.tc.beta_b, len(x)))          # float64 (:120-122)
        noise = torch.randn(x.shape, generator=generator, dtype=x.dtype)
        mask = torch.rand(y.size(0), generator=generator) < LABEL_DROPOUT
        return mix_noise(x, noise_level, noise), noise_level.float(), drop_labels(y, mask)

    def forward_backward(self, x_noisy: torch.Tensor, noise_level: torch.Tensor, label: torch.Tensor, target: torch.Tensor, *,
                         last_micro_batch: bool = True):
        """zero_grad + forward + MSE + backward (tld/train.py:163-168).  Returns (loss [1] on the device, pred); the gradients are in
        ``self.grads`` (flat) / ``grad_dict()``.

        Gradient accumulation (``accelerator.accumulate()``, tld/train.py:160, with ``gradient_accumulation_steps`` = n > 1): call n - 1 times
        with ``last_micro_batch=False`` and once with the default; ``optimizer_step()`` then steps on the MEAN of the n micro-batch gradients
        (equal micro-batch sizes: the gradient of the mean loss).  Like DDP's ``no_sync`` the ranks exchange nothing until the last micro-batch:
        the accumulated sum is reduced by ONE all-reduce in ``optimizer_step``."""
        dev = self.device
        t = lambda a: a.detach().to(dev, torch.float32).contiguous()
        xn, nl, lab, tgt = t(x_noisy), t(noise_level).view(-1), t(label), t(target)
        B = xn.shape[0]
        if not (nl.numel() == B and lab.shape[0] == B and tgt.shape == xn.shape):
            raise ValueError("inconsistent batch shapes")
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        accumulating = (not last_micro_batch) or self._acc_n > 0
        if self.use_graph and B == self.max_batch and self._world() > 1 and self.overlap_allreduce and not self._graph_world_warned:
            self._graph_world_warned = True
            warnings.warn("Trainer: HIP-graph replay is on with more than one rank -- full batches reduce their gradients with ONE all-reduce after the "
                          "backward instead of the per-block slices under it (use_graph=False / TLD_TRAIN_GRAPH=0 restores the overlap)", RuntimeWarning)
        overlap = self.overlap_allreduce and self._world() > 1 and not (self.use_graph and B == self.max_batch) and not accumulating
        self.wait_gradients()             # a previous call's slice reductions may still be running on the communication stream: they read / write self.grads
        self._slices = []
        self._cb_error = None
        self._reduced = False             # (a previous overlapped call that was never stepped on must not vouch for THIS call's gradients)
        cb = None
        if overlap:
            import torch.distributed as dist
            if self._comm_stream is None:
                self._comm_stream = torch.cuda.Stream(device=dev)
            compute = torch.cuda.current_stream(dev)

            def ready(_user, off, n):      # called by the engine, on this thread, right after the kernels finishing grads[off : off + n] are enqueued
                if self._cb_error is not None:
                    return                 # a slice already failed: the step is void, launch nothing more
                try:                       # ctypes swallows what a callback raises: keep it and re-raise when the engine call returns
                    ev = torch.cuda.Event()
                    ev.record(compute)
                    self._comm_stream.wait_event(ev)
                    with torch.cuda.stream(self._comm_stream):
                        self._pending.append(dist.all_reduce(self.grads[off:off + n], op=dist.ReduceOp.SUM, group=self.group, async_op=True))
                    self._slices.append((int(off), int(n)))
                except BaseException as e:  # noqa: BLE001 -- re-raised below
                    self._cb_error = e
            cb = _lib.GRAD_READY_FN(ready)

        def launch(xn_, nl_, lab_, tgt_, pred_, refresh=False):
            stream = torch.cuda.current_stream(dev).cuda_stream
            with torch.cuda.device(dev):
                if cb is not None:
                    _lib.check(_lib.lib().tld_train_forward_backward_cb(self._h, C.c_void_p(xn_.data_ptr()), C.c_void_p(nl_.data_ptr()), C.c_void_p(lab_.data_ptr()),
                                                                        C.c_void_p(tgt_.data_ptr()), B, C.c_void_p(self._loss.data_ptr()), C.c_void_p(pred_.data_ptr()),
                                                                        C.c_void_p(stream), cb, None), "tld_train_forward_backward_cb")
                    if self._cb_error is not None:
                        err, self._cb_error = self._cb_error, None
                        self._abandon_pending()
                        raise RuntimeError("gradient all-reduce of a slice failed during the backward; the step's gradients are not reduced") from err
                    self._reduced = True
                    return
                if refresh:     # graph capture: the bf16 / transposed operand copies are rebuilt INSIDE the captured region, whatever the engine's
                    # weights_fresh flag says at capture time -- every replay then follows the optimizer's latest parameters
                    _lib.check(_lib.lib().tld_train_refresh_weights(self._h, C.c_void_p(stream)), "tld_train_refresh_weights")
                _lib.check(_lib.lib().tld_train_forward_backward(self._h, C.c_void_p(xn_.data_ptr()), C.c_void_p(nl_.data_ptr()), C.c_void_p(lab_.data_ptr()),
                                                                 C.c_void_p(tgt_.data_ptr()), B, C.c_void_p(self._loss.data_ptr()), C.c_void_p(pred_.data_ptr()),
                                                                 C.c_void_p(stream)), "tld_train_forward_backward")
        if self.use_graph and B == self.max_batch and not self._debug:      # (a debug step is never captured: the hook copies and allocates)
            self._graph_calls += 1
            if self._graph_calls >= 2:
                if self._graph is None:      # second call: fixed buffers, capture (the first call ran eagerly: one-time attribute / cache set-up is done)
                    self._static = tuple(torch.empty_like(a) for a in (xn, nl, lab, tgt, xn))
                    for dst, src in zip(self._static[:4], (xn, nl, lab, tgt)):
                        dst.copy_(src)
                    torch.cuda.synchronize(dev)
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        launch(*self._static, refresh=True)
                    self._graph = g
                else:
                    for dst, src in zip(self._static[:4], (xn, nl, lab, tgt)):
                        dst.copy_(src)
                self._graph.replay()
                self._note_forward(B, self._static[1])
                return self._fold_micro_batch(last_micro_batch), self._static[4].clone()         # (a copy: the static buffer is overwritten by the next replay)
        pred = torch.empty_like(xn)
        launch(xn, nl, lab, tgt, pred)
        self._note_forward(B, nl)
        return self._fold_micro_batch(last_micro_batch), pred

    def _note_forward(self, B: int, nl: torch.Tensor) -> None:
        """After a forward_backward: remember its batch for ``sample_loss`` and, with ``loss_buckets``, add the step's per-sample losses to
        ``train_loss_levels`` at the step's own noise levels (two launches, outside the captured region)."""
        self._last_batch = B
        if self.train_loss_levels is not None:
            self._accumulate_levels(self.sample_loss(), nl, self.train_loss_levels)

    def _fold_micro_batch(self, last: bool) -> torch.Tensor:
        """Gradient accumulation bookkeeping after a forward_backward; returns the loss tensor to hand out (a copy while accumulating: the engine
        overwrites its loss cell on the next micro-batch).  ``global_step`` advances HERE, once per micro-batch: the reference counts loader
        iterations (``global_step += 1`` after every pass through ``accelerator.accumulate()``, tld/train.py:162-174), so checkpoints and the
        ``save_and_eval_every_iters`` cadence keep its meaning with accumulation on.  One stated deviation remains for n > 1 micro-batches: the
        reference calls ``update_ema`` in every iteration (on unchanged weights between optimizer steps), this trainer once per optimizer step."""
        self.global_step += 1
        if last and self._acc_n == 0:
            self._micro_scale = 1.0
            return self._loss
        if self._acc is None:
            self._acc = torch.zeros_like(self.grads)
        if last:                                  # grads <- sum of all micro-batch gradients; the optimizer kernel divides by their number
            self.grads.add_(self._acc)
            self._micro_scale = 1.0 / (self._acc_n + 1)
            self._acc.zero_(); self._acc_n = 0
        else:
            self._acc.add_(self.grads)
            self._acc_n += 1
        return self._loss.clone()

    def reset_accumulation(self) -> None:
        """Abandon a gradient accumulation in progress (an exception in a later micro-batch, a skipped bad batch): the folded gradients are
        dropped and the next forward_backward starts a fresh step.  Also called when weights or a checkpoint are loaded."""
        if self._acc is not None:
            self._acc.zero_()
        self._acc_n = 0
        self._micro_scale = 1.0

    def _world(self) -> int:
        import torch.distributed as dist
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def wait_gradients(self) -> None:
        """Make the current stream wait for every gradient-slice all-reduce still in flight (overlap mode).  Until then ``self.grads`` is a mix of
        local and summed slices; after it, it is the cross-rank SUM (the optimizer kernel applies 1 / world).  Called by ``grad_dict``,
        ``optimizer_step`` and at the start of the next ``forward_backward``; a no-op when nothing is pending."""
        pending, self._pending = self._pending, []
        for w in pending:
            w.wait()

    def _abandon_pending(self) -> None:
        pending, self._pending = self._pending, []
        for w in pending:
            try:
                w.wait()
            except Exception:      # noqa: BLE001 -- the step is already being abandoned with the first error
                pass
        self._reduced = False

    def _slices_tile_vector(self) -> bool:
        """True when the recorded slices cover [0, numel) exactly once (they arrive last block first; order does not matter here)."""
        pos = 0
        for off, n in sorted(self._slices):
            if off != pos:
                return False
            pos += n
        return pos == self.numel

    def optimizer_step(self) -> None:
        """DDP gradient mean + Adam + EMA (tld/train.py:168-172).  The gradient sum over the ranks is either already in flight (per-block slices
        started during the backward, ``overlap_allreduce``) or one all-reduce of the flat vector here.

        With ``max_grad_norm`` and / or ``skip_nonfinite`` the step is guarded on the device (``tld_train_grad_guard`` +
        ``tld_train_adam_ema_guarded``, no host synchronisation): the global norm is that of the MEAN gradient of the whole step -- taken
        after the all-reduce and after the accumulation over micro-batches, with the same 1 / world x 1 / micro-batches factor the optimizer
        applies -- so it is the same on every rank, and every rank clips (``torch.nn.utils.clip_grad_norm_`` semantics) or skips (a
        non-finite norm, as accelerate's ``GradScaler`` does) alike.  A skipped step changes nothing and does not advance Adam's bias
        correction: ``self.step`` keeps counting the calls, the device's count of APPLIED steps (``optimizer_stats()``) is what Adam uses."""
        if self._acc_n:
            raise RuntimeError(f"optimizer_step in the middle of a gradient accumulation ({self._acc_n} micro-batches folded, none marked last); "
                               "finish it with a forward_backward(last_micro_batch=True) or drop it with reset_accumulation()")
        if self._reduced:
            self._reduced = False
            self.wait_gradients()         # the current stream waits for the slices' reductions
            if not self._slices_tile_vector():
                raise RuntimeError(f"overlapped gradient all-reduce covered {sum(n for _, n in self._slices)} of {self.numel} elements: "
                                   "refusing to step on partly reduced gradients")
            scale = 1.0 / self._world()
        else:
            scale = allreduce_mean_(self.grads, self.group)
        scale *= self._micro_scale
        self._micro_scale = 1.0
        self.step += 1
        stream = torch.cuda.current_stream(self.device).cuda_stream
        p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
        if self.grouped:
            L = _lib.lib()
            b1, b2 = float(self.betas[0]), float(self.betas[1])
            with torch.cuda.device(self.device):
                _lib.check(L.tld_train_grad_guard_grouped(self._plan, p(self.grads), self.numel, float(scale),
                                                          self.max_grad_norm if self.max_grad_norm is not None else 0.0, int(self.skip_nonfinite), b1, b2,
                                                          p(self._opt_state), C.c_void_p(stream)), "tld_train_grad_guard_grouped")
                _lib.check(L.tld_train_adamw_ema_grouped(self._plan, p(self.params), p(self.grads), p(self.exp_avg), p(self.exp_avg_sq), p(self.ema),
                                                         self.numel, float(self.tc.lr), b1, b2, float(self.eps), float(self.tc.alpha), float(scale),
                                                         p(self._opt_state), C.c_void_p(stream)), "tld_train_adamw_ema_grouped")
                # the grouped entries take no engine: binding the same vectors again marks its bf16 operand copies stale
                _lib.check(L.tld_train_bind(self._h, p(self.params), p(self.grads)), "tld_train_bind")
            return
        if self.guarded:
            L = _lib.lib()
            b1, b2 = float(self.betas[0]), float(self.betas[1])
            with torch.cuda.device(self.device):
                _lib.check(L.tld_train_grad_guard(self._h, p(self.grads), self.numel, float(scale), self.max_grad_norm if self.max_grad_norm is not None else 0.0,
                                                  int(self.skip_nonfinite), b1, b2, p(self._opt_state), C.c_void_p(stream)), "tld_train_grad_guard")
                _lib.check(L.tld_train_adam_ema_guarded(self._h, p(self.params), p(self.grads), p(self.exp_avg), p(self.exp_avg_sq), p(self.ema), self.numel,
                                                        float(self.tc.lr), b1, b2, float(self.eps), float(self.tc.alpha), float(scale), p(self._opt_state),
                                                        C.c_void_p(stream)), "tld_train_adam_ema_guarded")
            return
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_train_adam_ema(self._h, p(self.params), p(self.grads), p(self.exp_avg), p(self.exp_avg_sq), p(self.ema), self.numel,
                                                     float(self.tc.lr), float(self.betas[0]), float(self.betas[1]), float(self.eps), self.step,
                                                     float(self.tc.alpha), float(scale), C.c_void_p(stream)), "tld_train_adam_ema")

    # ---- the guard's readouts ----------------------------------------------------------------------------------------------------
    def _need_guard(self) -> None:
        if self._opt_state is None:
            raise RuntimeError("this Trainer's optimizer step is not guarded (construct it with max_grad_norm= and / or skip_nonfinite=True)")

    @property
    def tensor_grad_norms(self) -> torch.Tensor:
        """Per-tensor norms of the last step's mean gradient, fp64 ``[n_tensors]`` on the device in ``param_layout`` order (frozen tensors
        included; before clipping): the square roots of the plan's per-segment sums -- reading it does not synchronise.  Grouped trainers only."""
        if self._plan is None:
            raise RuntimeError("this Trainer's optimizer step is not grouped (construct it with weight_decay=, param_groups= or lr_schedule=)")
        return self._seg_sq.sqrt()

    @property
    def grad_norm(self) -> torch.Tensor:
        """Global norm of the last step's mean gradient (before clipping; Inf or NaN when non-finite): a 0-d fp64 view of the device state --
        reading the attribute does not synchronise, ``float()`` of it does."""
        self._need_guard()
        return self._opt_state[3]

    def optimizer_stats(self) -> Dict[str, object]:
        """Synchronises and returns the guard's state: ``grad_norm``, ``clip_coef``, ``applied_steps``, ``skipped_steps``, ``last_skipped``."""
        self._need_guard()
        t, skipped, last, norm, coef, _, _, factor = self._opt_state[:8].cpu().tolist()
        out = {"grad_norm": norm, "clip_coef": coef, "applied_steps": int(t), "skipped_steps": int(skipped), "last_skipped": bool(last)}
        if self.grouped:                  # the schedule factor of the last applied step (1 without a schedule, 0 before the first step)
            out["lr_factor"] = factor
        return out

    def _factor_at(self, t: int) -> float:
        """The schedule factor applied step ``t`` >= 1 runs at: ``table[min(t, n) - 1]``, or 1 without a table."""
        return 1.0 if self._lr_table is None else float(self._lr_table[min(int(t), self._lr_table.size) - 1])

    def _set_applied_steps(self, t: int) -> None:
        """The guard's state for an optimizer that has applied ``t`` steps (tld_train_grad_guard's formula, float-rounded betas in double)."""
        st = torch.zeros(_lib.TRAIN_OPT_STATE_DOUBLES, dtype=torch.float64)
        b1, b2 = (float(np.float32(b)) for b in self.betas)
        st[0], st[5], st[6] = float(t), 1.0 - b1 ** t, 1.0 - b2 ** t
        if self.grouped and t > 0:
            st[7] = self._factor_at(t)
        self._opt_state.copy_(st)

    def train_step(self, x: torch.Tensor, y: torch.Tensor, np_rng: Optional[np.random.Generator] = None,
                   generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """One iteration of the reference's inner loop on the batch (x, y) as the loader yields it (x already divided by the VAE scale
        factor, :119).  Returns the loss tensor (device, not synchronised)."""
        x_noisy, noise_level, label = self.make_batch(x, y, np_rng, generator)
        staged = self._stage_batch((x_noisy, noise_level, label, x))
        loss, _ = self.forward_backward(*staged)
        self._release_stage()
        self.optimizer_step()
        return loss

    # ---- the device data path --------------------------------------------------------------------------
    @property
    def bad_indices(self) -> torch.Tensor:
        """How many row indices ``prepare_batch``'s kernel has refused since this trainer was built (each such position trained on row 0): a 0-d
        int32 view of the device counter -- reading the attribute does not synchronise, ``int()`` of it does."""
        return self._bad[0]

    def _rank(self) -> int:
        import torch.distributed as dist
        return dist.get_rank(self.group) if dist.is_available() and dist.is_initialized() else 0

    def prepare_batch(self, dataset, idx, *, step: Optional[int] = None, debug: bool = False):
        """``make_batch`` on the device (tld/train.py:121-138): rows ``idx`` of a ``data.DeviceLatentDataset`` -> ``(x_noisy, noise_level, label,
        target)``, fp32 device tensors ready for ``forward_backward``; one kernel on the current stream, no host wait.  The noise, the Beta noise
        level and the label mask are Philox draws keyed by ``data_seed`` and addressed by (rank, ``step``, position): ``step`` defaults to
        ``global_step``, which a checkpoint carries, so a resumed run continues the stream of the uninterrupted one.  A host ``idx`` (list, array,
        CPU tensor) is range-checked here; a device ``idx`` is left to the kernel's guard (``bad_indices``).  ``debug=True`` appends
        ``(noise, noise_level64, mask)``, what was drawn."""
        dev = self.device
        if dataset.device.type != "cuda" or (dataset.device.index if dataset.device.index is not None else torch.cuda.current_device()) != dev.index:
            raise ValueError(f"the dataset lives on {dataset.device}, this trainer on {dev}")
        shape = (self.cfg.n_channels, self.cfg.image_size, self.cfg.image_size)
        if tuple(dataset.sample_shape) != shape or dataset.text_emb.shape[1] != self.cfg.text_emb_size:
            raise ValueError(f"dataset rows are {tuple(dataset.sample_shape)} with {dataset.text_emb.shape[1]} text features; the model takes {shape} and "
                             f"{self.cfg.text_emb_size}")
        if not (isinstance(idx, torch.Tensor) and idx.device.type == "cuda"):
            host = torch.as_tensor(idx).reshape(-1)
            if host.numel() and (host.dtype.is_floating_point or int(host.min()) < 0 or int(host.max()) >= len(dataset)):
                raise IndexError(f"batch indices outside [0, {len(dataset)}) (or not integers)")
            idx = host
        idx = idx.reshape(-1).to(dev, torch.int64).contiguous()
        B = int(idx.numel())
        if B == 0:
            raise ValueError("an empty batch")
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        x_noisy, noise_level, label, target = f(B, *shape), f(B), f(B, self.cfg.text_emb_size), f(B, *shape)
        extra = (f(B, *shape), torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)) if debug else (None, None, None)
        src = dataset.source()
        p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().tld_train_prepare_batch(self._h, C.byref(src), p(idx), B, self.data_seed, int(self.global_step if step is None else step),
                                                          self._rank(), float(self.tc.beta_a), float(self.tc.beta_b), LABEL_DROPOUT, p(x_noisy),
                                                          p(noise_level), p(label), p(target), p(extra[0]), p(extra[1]), p(extra[2]), p(self._bad),
                                                          C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "tld_train_prepare_batch")
        out = (x_noisy, noise_level, label, target)
        return out + (extra[0], extra[1], extra[2].bool()) if debug else out

    def train_step_from(self, dataset, idx) -> torch.Tensor:
        """``train_step`` without the host: ``prepare_batch`` + ``forward_backward`` + ``optimizer_step`` on rows ``idx`` of a device-resident
        dataset.  Returns the loss tensor (device, not synchronised).  With graph replay on, the prepared tensors go through the captured step's
        fixed input buffers like any other device batch."""
        loss, _ = self.forward_backward(*self.prepare_batch(dataset, idx))
        self.optimizer_step()
        return loss

    def _stage_batch(self, arrs):
        """Host tensors -> device through pinned double buffers on a copy stream (see __init__); device tensors pass through."""
        if not all(isinstance(a, torch.Tensor) and a.device.type == "cpu" for a in arrs):
            return arrs
        dev = self.device
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=dev)
        i = self._stage_i = self._stage_i ^ 1
        shapes = tuple(tuple(a.shape) for a in arrs)
        st = self._stage[i]
        compute = torch.cuda.current_stream(dev)
        if st is None or st["shapes"] != shapes:
            # the device buffers are allocated ON the copy stream: the caching allocator recycles blocks per stream, and a block just released by the
            # compute stream (say the previous step's prediction copy, its kernel still queued) must not come back here and be written by the copy
            # stream ahead of that kernel -- the first version of this did exactly that and trained on a corrupted batch
            with torch.cuda.stream(self._copy_stream):
                devb = [torch.empty(a.shape, dtype=torch.float32, device=dev) for a in arrs]
            for t_ in devb:
                t_.record_stream(compute)
            st = {"shapes": shapes, "host": [torch.empty(a.shape, dtype=torch.float32).pin_memory() for a in arrs], "dev": devb, "copied": None, "free": None}
            self._stage[i] = st
        if st["copied"] is not None:
            st["copied"].synchronize()            # the copy that last read these pinned buffers (two steps ago: long done)
        for h, a in zip(st["host"], arrs):
            h.copy_(a)
        if st["free"] is not None:
            self._copy_stream.wait_event(st["free"])      # the step that last read these device buffers has finished with them
        with torch.cuda.stream(self._copy_stream):
            for d, h in zip(st["dev"], st["host"]):
                d.copy_(h, non_blocking=True)
            st["copied"] = torch.cuda.Event()
            st["copied"].record(self._copy_stream)
        compute.wait_event(st["copied"])
        return tuple(st["dev"])

    def _release_stage(self):
        st = self._stage[self._stage_i]
        if st is not None:
            st["free"] = torch.cuda.Event()
            st["free"].record(torch.cuda.current_stream(self.device))

    # ---- held-out loss, per sample and by noise level ----------------------------------------------------
    def _loss_weights(self, weights) -> Optional[torch.Tensor]:
        """``"model"`` -> None (the bound parameters), ``"ema"`` -> the EMA vector, or a flat fp32 device vector of ``numel`` elements."""
        if isinstance(weights, str):
            if weights in ("model", "live"):
                return None
            if weights == "ema":
                return self._weights_vector("ema")
            raise ValueError(f"weights = {weights!r}: 'model', 'ema' or a flat tensor")
        if not isinstance(weights, torch.Tensor):
            raise TypeError("weights: 'model', 'ema' or a flat float32 tensor on the trainer's device")
        if weights.dtype != torch.float32 or weights.device != self.device or weights.numel() != self.numel or not weights.is_contiguous():
            raise ValueError(f"a weight vector must be contiguous float32 [{self.numel}] on {self.device}")
        return weights

    def _forward_loss(self, xn, nl, lab, tgt, wvec, loss, sample, pred) -> None:
        B = int(xn.shape[0])
        p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_train_forward_loss(self._h, p(wvec), p(xn), p(nl), p(lab), p(tgt), B, p(loss), p(sample), p(pred),
                                                         C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "tld_train_forward_loss")
        self._last_batch = B

    def forward_loss(self, x_noisy: torch.Tensor, noise_level: torch.Tensor, label: torch.Tensor, target: torch.Tensor, *, weights="model"):
        """The forward half of ``forward_backward`` on the live parameters (``"model"``), the EMA copy (``"ema"``) or any flat weight vector:
        returns ``(loss [1], sample_loss fp64 [B], pred)`` on the device.  Same kernels, same bits as the training forward; it writes no gradient,
        advances no counter and leaves an accumulation in progress alone.  The loss is a tensor of its own (not the training step's cell)."""
        dev = self.device
        t = lambda a: a.detach().to(dev, torch.float32).contiguous()
        xn, nl, lab, tgt = t(x_noisy), t(noise_level).view(-1), t(label), t(target)
        B = xn.shape[0]
        if not (nl.numel() == B and lab.shape[0] == B and tgt.shape == xn.shape):
            raise ValueError("inconsistent batch shapes")
        if B > self.max_batch:
            raise ValueError(f"batch {B} exceeds max_batch {self.max_batch}")
        wvec = self._loss_weights(weights)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        sample = torch.empty(B, dtype=torch.float64, device=dev)
        pred = torch.empty_like(xn)
        self._forward_loss(xn, nl, lab, tgt, wvec, loss, sample, pred)
        return loss, sample, pred

    def sample_loss(self) -> torch.Tensor:
        """Per-sample MSE (fp64 ``[B]``, summed in double in a fixed order) of the last ``forward_backward`` or ``forward_loss``, from the row errors
        the engine still holds -- after a graph replay too, which fills the same buffer."""
        if self._last_batch <= 0:
            raise RuntimeError("sample_loss: no forward has run yet")
        out = torch.empty(self._last_batch, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_train_sample_loss(self._h, None, self._last_batch, 0, 0, C.c_void_p(out.data_ptr()),
                                                        C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "tld_train_sample_loss")
        return out

    def _accumulate_levels(self, sample: torch.Tensor, nl: torch.Tensor, acc: EvalLoss) -> None:
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_train_loss_buckets(C.c_void_p(sample.data_ptr()), C.c_void_p(nl.data_ptr()), int(sample.numel()), acc.n_buckets,
                                                         C.c_void_p(acc.state.data_ptr()), C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
                       "tld_train_loss_buckets")

    def reset_loss_levels(self) -> None:
        """Zero ``train_loss_levels`` (``Trainer(loss_buckets=n)``)."""
        if self.train_loss_levels is None:
            raise RuntimeError("this Trainer keeps no training loss by noise level (construct it with loss_buckets=n)")
        self.train_loss_levels.zero_()

    def eval_loss(self, dataset, idx, *, weights="ema", noise_levels=None, n_buckets: int = 10, batch_size: Optional[int] = None,
                  seed: Optional[int] = None, reduce: bool = True) -> EvalLoss:
        """Held-out loss of rows ``idx`` of a ``data.DeviceLatentDataset`` by noise level, on the device and without a host wait.  The evaluation
        is a fixed sequence of batches ``idx[j B : (j + 1) B]`` (``B = batch_size or max_batch``, the last one may be short); position ``p``
        gets the level ``noise_levels[p % L]`` (default: the ``n_buckets`` bin midpoints); batch ``j`` is built by ``tld_train_prepare_batch_at`` with
        key ``seed`` (default ``data_seed ^ EVAL_SEED_XOR``), replica 0, step ``j`` and no label dropout, run through ``forward_loss`` on
        ``weights`` and added to the accumulator.  With more than one rank, rank ``r`` takes the batches ``j = r (mod world)`` and ``reduce=True``
        sums the state with one all-reduce: the result is a function of (weights, dataset, idx, B, levels, seed) and not of the world size, up to
        the order of a few double additions.  Nothing of the training step moves: ``global_step``, ``step``, gradients, an accumulation in
        progress and pending reductions stay as they are, and the launches are eager (never captured)."""
        dev = self.device
        if dataset.device.type != "cuda" or (dataset.device.index if dataset.device.index is not None else torch.cuda.current_device()) != dev.index:
            raise ValueError(f"the dataset lives on {dataset.device}, this trainer on {dev}")
        shape = (self.cfg.n_channels, self.cfg.image_size, self.cfg.image_size)
        if tuple(dataset.sample_shape) != shape or dataset.text_emb.shape[1] != self.cfg.text_emb_size:
            raise ValueError(f"dataset rows are {tuple(dataset.sample_shape)} with {dataset.text_emb.shape[1]} text features; the model takes {shape} and "
                             f"{self.cfg.text_emb_size}")
        if not (isinstance(idx, torch.Tensor) and idx.device.type == "cuda"):
            host = torch.as_tensor(idx).reshape(-1)
            if host.numel() and (host.dtype.is_floating_point or int(host.min()) < 0 or int(host.max()) >= len(dataset)):
                raise IndexError(f"evaluation indices outside [0, {len(dataset)}) (or not integers)")
            idx = host
        idx = idx.reshape(-1).to(dev, torch.int64).contiguous()
        n = int(idx.numel())
        if n == 0:
            raise ValueError("an empty evaluation set")
        B = int(batch_size) if batch_size is not None else self.max_batch
        if not 1 <= B <= self.max_batch:
            raise ValueError(f"batch_size {B} outside [1, max_batch = {self.max_batch}]")
        out = EvalLoss(n_buckets, dev)
        levels = np.asarray(noise_levels, dtype=np.float64).reshape(-1) if noise_levels is not None else bucket_midpoints(out.n_buckets)
        plan = eval_plan(n, B, self._world(), self._rank(), levels)          # (refuses levels outside [0, 1])
        wvec = self._loss_weights(weights)
        key = (self.data_seed ^ EVAL_SEED_XOR if seed is None else int(seed)) & (2 ** 64 - 1)
        # the level table goes up once, from pinned memory: the copy is ordered on the stream and the host does not wait for it
        table = torch.from_numpy(np.ascontiguousarray(levels)).pin_memory().to(dev, non_blocking=True)
        level_at = table[torch.arange(n, device=dev) % table.numel()]
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
        x_noisy, noise_level, label, target = f(B, *shape), f(B), f(B, self.cfg.text_emb_size), f(B, *shape)
        loss, sample = f(1), torch.empty(B, dtype=torch.float64, device=dev)
        src = dataset.source()
        p = lambda a: C.c_void_p(a.data_ptr())
        L = _lib.lib()
        for j, start, stop, _ in plan:
            b = stop - start
            with torch.cuda.device(dev):
                _lib.check(L.tld_train_prepare_batch_at(self._h, C.byref(src), p(idx[start:stop]), b, key, j, 0, float(self.tc.beta_a), float(self.tc.beta_b),
                                                        0.0, p(x_noisy), p(noise_level), p(label), p(target), None, None, None, p(self._bad),
                                                        C.c_void_p(torch.cuda.current_stream(dev).cuda_stream), p(level_at[start:stop])),
                           "tld_train_prepare_batch_at")
            self._forward_loss(x_noisy[:b], noise_level[:b], label[:b], target[:b], wvec, loss, sample[:b], None)
            self._accumulate_levels(sample[:b], noise_level[:b], out)
        if reduce and self._world() > 1:
            import torch.distributed as dist
            dist.all_reduce(out.state, op=dist.ReduceOp.SUM, group=self.group)
        return out

    # ---- evaluation while training (tld/train.py:23-40,140-147) --------------------------------------------------------------------
    def _weights_vector(self, weights: str) -> torch.Tensor:
        if weights == "ema":
            if self.ema is None:
                raise RuntimeError("this Trainer keeps no EMA copy (keep_ema=False): evaluate weights='live'")
            return self.ema
        if weights == "live":
            return self.params
        raise ValueError(f"weights = {weights!r}: 'ema' or 'live'")

    def make_denoiser(self, model_batch: int = 32, weights: str = "ema"):
        """An inference ``Denoiser`` of this trainer's config on its device, reserved for ``model_batch`` samples per forward (the CFG-doubled
        count: 32 = the 16 images of the reference's ``eval_gen``), holding the EMA (``"ema"``) or the live (``"live"``) weights and this
        trainer's ``angular_speeds``.  ``sync_denoiser`` brings it up to date later without rebuilding it."""
        from .denoiser import Denoiser
        src = self._weights_vector(weights)
        den = Denoiser(**asdict(self.cfg)).to(self.device)
        den.load_state_dict({"fourier_feats.0.angular_speeds": self._angular.clone()}, strict=False)
        den.load_flat(src)
        return den.reserve(model_batch)

    def sync_denoiser(self, den, weights: str = "ema"):
        """``den.load_flat(self.ema or self.params)``: the denoiser's engine takes the trainer's current weights in place, by kernels on the current
        stream -- ordered behind the optimizer kernel that wrote them, with no device-to-host copy, no engine rebuild and no host wait."""
        den.load_flat(self._weights_vector(weights))
        return den

    @torch.no_grad()
    def eval_generate(self, labels: torch.Tensor, vae=None, *, num_imgs: int = 16, class_guidance: float = 4.5, seed: int = 10, n_iter: int = 40,
                      exponent: float = 1, sharp_f: float = 0.1, bright_f: float = 0.1, weights: str = "ema", model_batch: Optional[int] = None):
        """The reference's ``eval_gen`` (tld/train.py:23-35; defaults as there) from the weights this trainer holds NOW: a cached denoiser is synced
        (``sync_denoiser``) and samples ``num_imgs`` latents for ``repeat_interleave(labels, 2, dim=0)`` through
        ``DiffusionGenerator.generate_latents``.  Returns the latents, or ``(latents, images)`` with the decoded images of ``vae`` (an object
        with ``.decode``) when one is given.  Runs on the calling rank only, issues no collective, and touches nothing of the training step's
        state (gradients, accumulation, ``global_step``, the captured graph)."""
        from .diffusion import DiffusionGenerator
        need = int(model_batch) if model_batch is not None else 2 * int(num_imgs)
        key = str(weights)
        self._weights_vector(key)                 # (refusals before anything is built)
        if self._eval_den is None:
            self._eval_den = self.make_denoiser(need, key)
        else:
            self.sync_denoiser(self._eval_den.reserve(need), key)
        gen = DiffusionGenerator(self._eval_den, vae, self.device, torch.float32)
        latents = gen.generate_latents(labels=torch.repeat_interleave(labels, 2, dim=0), n_iter=n_iter, num_imgs=num_imgs, class_guidance=class_guidance,
                                       seed=seed, img_size=self.cfg.image_size, sharp_f=sharp_f, bright_f=bright_f, exponent=exponent)
        if vae is None:
            return latents
        return latents, gen._decode(latents, 8)[0]

    @torch.no_grad()
    def eval_clip_score(self, labels: torch.Tensor, vae, clip_image, **eval_generate_kwargs):
        """``eval_generate`` plus the CLIP score of every sample against the label it was generated from: the decoded images go from [-1, 1] to
        [0, 1], through ``clip_preprocess`` and ``clip_image.encode_image`` (a ``ClipImageEncoder`` or a ``Clip``), and ``clip_score`` takes the cosine
        with ``repeat_interleave(labels, 2, dim=0)[i]`` -- the labels are CLIP text embeddings, so no text tower runs.  Returns
        ``(latents, images, scores)``; ``scores`` is a ``[num_imgs]`` fp32 tensor on the trainer's device and is not synchronised here.  Touches
        nothing of the training step's state, like ``eval_generate``."""
        from .clip_image import clip_preprocess, clip_score
        if vae is None:
            raise ValueError("eval_clip_score needs a vae: the score is taken on decoded images")
        latents, images = self.eval_generate(labels, vae, **eval_generate_kwargs)
        size = getattr(clip_image, "visual", clip_image).input_resolution
        pixels = clip_preprocess((images.to(self.device, torch.float32) * 0.5 + 0.5).clamp(0.0, 1.0), size)
        emb = clip_image.encode_image(pixels)
        used = torch.repeat_interleave(labels, 2, dim=0)[:emb.shape[0]].to(self.device)
        return latents, images, clip_score(emb, used)

    @torch.no_grad()
    def eval_features(self, labels: torch.Tensor, vae, clip_image, bank, **eval_generate_kwargs):
        """``eval_generate`` plus the CLIP image embedding of every sample, appended to ``bank`` (a ``metrics.FeatureBank``): the decoded images go
        from [-1, 1] to [0, 1], through ``clip_preprocess`` and ``clip_image.encode_image`` -- the chain of ``eval_clip_score`` -- and ``bank.add``
        stores them (L2-normalised if the bank says so) with no host synchronisation.  Returns ``(latents, images)``.  Call it in a loop over label
        batches and seeds to fill a bank, then ``metrics.cmmd`` / ``metrics.frechet_distance`` against a bank of real images
        (``DiffusionTransformer.image_features``).  This rank's samples only: gathering banks across ranks is left to the caller.  Touches nothing
        of the training step's state, like ``eval_generate``."""
        from .metrics import image_embeddings
        if vae is None:
            raise ValueError("eval_features needs a vae: the embeddings are taken on decoded images")
        latents, images = self.eval_generate(labels, vae, **eval_generate_kwargs)
        bank.add(image_embeddings(clip_image, (images.to(self.device, torch.float32) * 0.5 + 0.5).clamp(0.0, 1.0), self.device))
        return latents, images

    # ---- checkpoint / resume ----------------------------------------------------------------------------------------------------
    def optimizer_state_dict(self) -> Dict[str, object]:
        """``torch.optim.Adam(model.parameters(), lr).state_dict()`` as the reference saves it (tld/train.py:86,152): per-parameter
        ``{step, exp_avg, exp_avg_sq}`` in ``named_parameters()`` order + one param group.  (Before the first step torch's ``state`` is empty.)"""
        state = {}
        step = self.optimizer_stats()["applied_steps"] if self.guarded or self.grouped else self.step      # (a checkpoint copies everything to the host anyway)
        if step > 0:
            for i, (k, (o, s)) in enumerate(self.layout.items()):
                if self.grouped and self._groups[self._seg_group[i]][2]:
                    continue              # a frozen tensor has no Adam state, as a parameter with requires_grad = False has none in torch
                n = int(np.prod(s))
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": self.exp_avg[o:o + n].view(*s).clone(),
                            "exp_avg_sq": self.exp_avg_sq[o:o + n].view(*s).clone()}
        if self.grouped:                  # torch.optim.AdamW's groups; lr as LambdaLR leaves it after `step` steps: that of the NEXT step
            return {"state": state, "param_groups": opt_groups.torch_param_groups(self._seg_group, self._groups, self.tc.lr, self.betas, self.eps,
                                                                                  self._factor_at(step + 1), self._lr_table is not None)}
        group = {"lr": self.tc.lr, "betas": tuple(self.betas), "eps": self.eps, "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "params": list(range(len(self.layout)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, osd: Mapping[str, object]) -> None:
        """Inverse of ``optimizer_state_dict`` (``optimizer.load_state_dict`` of tld/train.py:100): also accepts a reference checkpoint's Adam state."""
        state = osd.get("state", {})
        groups = osd.get("param_groups") or []
        if self.grouped:                  # refused before anything is touched
            mine = [[i for i, q in enumerate(self._seg_group) if q == k] for k in range(len(self._groups))]
            theirs = [[int(i) for i in g.get("params", [])] for g in groups]
            if theirs != mine:
                raise RuntimeError(f"the checkpoint's optimizer has {len(theirs)} param groups over another partition of the parameters than this "
                                   f"trainer's {len(mine)} groups")
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        steps = set()
        for i, (k, (o, s)) in enumerate(self.layout.items()):
            st = state.get(i, state.get(str(i)))
            if st is None:
                continue
            n = int(np.prod(s))
            for name, flat in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
                t = torch.as_tensor(st[name]).detach().to(torch.float32)
                if tuple(t.shape) != s:
                    raise RuntimeError(f"optimizer state of parameter {i} ({k}): shape {tuple(t.shape)}, expected {s}")
                flat[o:o + n].copy_(t.reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise RuntimeError(f"per-parameter Adam step counts differ ({sorted(steps)}): the fused optimizer kernel keeps one count")
        self.step = steps.pop() if steps else 0
        if groups:
            self.tc.lr = float(groups[0].get("initial_lr", groups[0].get("lr", self.tc.lr)) if self.grouped else groups[0].get("lr", self.tc.lr))
            self.betas = tuple(groups[0].get("betas", self.betas)); self.eps = float(groups[0].get("eps", self.eps))
        if self.guarded or self.grouped:      # the device's count restarts from the checkpoint's applied steps; skips are not carried
            self._set_applied_steps(self.step)

    def checkpoint(self) -> Dict[str, object]:
        """The dict the reference saves (tld/train.py:150-156): EMA weights, ``optimizer.state_dict()``, global step."""
        return {"model_ema": self.ema_state_dict(), "opt_state": self.optimizer_state_dict(), "global_step": self.global_step}

    def load_checkpoint(self, ckpt) -> "Trainer":
        """Resume as the reference does with ``from_scratch=False`` (tld/train.py:92-104): the EMA weights go into the live model (and the EMA
        copy restarts from them), the optimizer state and the step count are restored.  ``ckpt``: the dict, or a path to a torch-saved one."""
        if isinstance(ckpt, (str, os.PathLike)):
            ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
        sd = {k.replace("_orig_mod.", "").replace("module.", ""): v for k, v in ckpt["model_ema"].items()}
        self.load_state_dict(sd)
        self.load_optimizer_state_dict(ckpt["opt_state"])
        # the loop counter and Adam's bias-correction count are different things: a checkpoint saved before the first optimizer step of a
        # resumed run (empty Adam state) keeps Adam at step 0 -- fresh moments with step = global_step would be under-corrected
        self.global_step = int(ckpt.get("global_step", self.step))
        return self

"""``Denoiser``: the reference's model object, backed by the gfx950 engine.

Keeps the constructor and call contract the reference's sampler, pipeline and tests rely on
(reference tld/denoiser.py:85-126):

    Denoiser(**asdict(DenoiserConfig()))            ctor kwargs = the nine config fields
    model(x, noise_level, label) -> x0_pred         [B,C,S,S], [B,1], [B,text] -> [B,C,S,S]
    model.eval() / .to(dtype) / .to(device)         chainable
    model.load_state_dict(sd) / .state_dict()       reference key names and shapes
    model.load_flat(flat)                           the parameters as one fp32 vector (``weights.param_layout`` order); a live engine is refreshed in place
    model.parameters()                              fp32 tensors (count matches the reference)
    model.n_channels, model.image_size              ints

Arithmetic runs in ``libtld_hip.so`` (bf16 MFMA operands, fp32 accumulation, bf16 residual stream --
fp32 when built with ``-DTLD_RESID_FP32`` -- and fp32 conditioning path); Python owns configuration,
weight hand-over and tensors only.  There is no
CPU or eager-PyTorch fallback: calling the model without a HIP device raises.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import OrderedDict
from typing import Dict, Iterator, Optional

import numpy as np
import torch

from . import _lib
from .weights import param_count, param_layout, state_dict_spec, synth_state_dict

_IO_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.bfloat16: _lib.DTYPE_BF16, torch.float16: _lib.DTYPE_F16}


class Denoiser:
    def __init__(self, image_size: int, noise_embed_dims: int, patch_size: int, embed_dim: int, dropout: float,
                 n_layers: int, text_emb_size: int = 768, mlp_multiplier: int = 4, n_channels: int = 4,
                 init_seed: int = 0):
        self.image_size = image_size
        self.noise_embed_dims = noise_embed_dims
        self.patch_size = patch_size
        self.embed_dim = embed_dim
        self.dropout = dropout            # identity at inference (eval mode is the only mode)
        self.n_layers = n_layers
        self.text_emb_size = text_emb_size
        self.mlp_multiplier = mlp_multiplier
        self.n_channels = n_channels
        self._cfg = dict(image_size=image_size, noise_embed_dims=noise_embed_dims, patch_size=patch_size,
                         embed_dim=embed_dim, dropout=dropout, n_layers=n_layers, text_emb_size=text_emb_size,
                         n_channels=n_channels, mlp_multiplier=mlp_multiplier)
        self._spec = state_dict_spec(self._cfg)
        self.param_count = param_count(self._cfg)     # length of the flat parameter vector (load_flat)
        # the engine's weights when they came through load_flat: a private device copy of the vector.  While _flat_stale is set the host state below is
        # behind it, and the first reader of self._state brings it up to date (one device-to-host copy)
        self._flat: Optional[torch.Tensor] = None
        self._flat_stale = False
        # like nn.Module construction, a fresh model holds (deterministic) random weights
        self._state = OrderedDict((k, torch.from_numpy(np.array(v))) for k, v in synth_state_dict(self._cfg, init_seed).items())
        self._device: Optional[torch.device] = None
        self._dtype = torch.float32
        self._engine = None
        self._engine_batch = 0
        self._engine_device = None
        self._engine_skip = True          # the engine's TLD_GUIDANCE_SKIP, as tld_engine_create read it
        self._gemm_dtype = 0              # 0: bf16 operands; 1: MX-fp8 QKV / MLP GEMMs (set_gemm_dtype)
        self._low_latency = 0             # capacity class for small batches (set_low_latency): 0 default, 1 / 2 = split-K down projection in four / eight splits
        self._session = None              # the sampler session open on the engine (open_session), or None
        self.training = False

    # ---- nn.Module-like surface ------------------------------------------------------------------
    def eval(self) -> "Denoiser":
        self.training = False
        return self

    def train(self, mode: bool = True) -> "Denoiser":
        if mode:
            raise NotImplementedError("this object is the inference engine; the training step (tld/train.py:118-175) is transformer_latent_diffusion_amd.Trainer")
        return self.eval()

    def to(self, *args, **kwargs) -> "Denoiser":
        for a in list(args) + list(kwargs.values()):
            if isinstance(a, torch.dtype):
                if a not in _IO_DTYPES:
                    raise TypeError(f"unsupported model dtype {a}")
                self._dtype = a
            elif isinstance(a, (torch.device, str)):
                dev = torch.device(a)
                if dev != self._device:
                    self._drop_engine()
                self._device = dev
        return self

    def cuda(self, index: int = 0) -> "Denoiser":
        return self.to(torch.device("cuda", index))

    def parameters(self) -> Iterator[torch.Tensor]:
        for k, (shape, kind) in self._spec.items():
            if kind not in ("angular", "arange"):
                yield self._state[k]

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return OrderedDict((k, v.clone()) for k, v in self._state.items())

    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True):
        missing = [k for k in self._spec if k not in sd]
        unexpected = [k for k in sd if k not in self._spec]
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for Denoiser: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        new = OrderedDict(self._state)
        for k, (shape, kind) in self._spec.items():
            if k not in sd:
                continue
            t = torch.as_tensor(sd[k]).detach().cpu()
            if tuple(t.shape) != tuple(shape):
                raise RuntimeError(f"size mismatch for {k}: copying a param with shape {tuple(t.shape)}, "
                                   f"the shape in current model is {tuple(shape)}")
            new[k] = t.to(torch.int64 if kind == "arange" else torch.float32).contiguous().clone()
        self._state = new
        self._drop_engine()
        return self

    # the host state: {key: fp32 tensor} under the reference's keys.  Assigning it (load_state_dict, the constructor) makes it current; after a
    # load_flat into a live engine it is materialised from the device copy on first use -- by state_dict(), parameters() or an engine rebuild
    @property
    def _state(self) -> "OrderedDict[str, torch.Tensor]":
        if self._flat_stale:
            self._host_state = self._state_from_flat(self._flat.cpu())
            self._flat_stale = False
        return self._host_state

    @_state.setter
    def _state(self, value):
        self._host_state = value
        self._flat_stale = False

    def _state_from_flat(self, host_flat: torch.Tensor) -> "OrderedDict[str, torch.Tensor]":
        """The host state with its parameters taken from ``host_flat``; the two registered buffers keep their values."""
        new = OrderedDict(self._host_state)
        for k, (o, shape) in param_layout(self._cfg).items():
            new[k] = host_flat[o:o + int(np.prod(shape))].view(*shape).clone()
        return new

    def load_flat(self, flat: torch.Tensor) -> "Denoiser":
        """The parameters from ONE fp32 vector of ``param_count`` elements in ``weights.param_layout`` order (``weights.flatten_state_dict``;
        a ``Trainer``'s ``params`` / ``ema``), on the CPU or on the engine's device.  ``angular_speeds`` is not a parameter and keeps its value.

        With a live engine its weight images are rebuilt in place by kernels on the current stream (``tld_engine_refresh_weights``: bit-equal to
        a load of the same values through ``load_state_dict``): the engine, its capacity, GEMM dtype, low-latency class and debug / profile state
        stay, nothing is rebuilt and nothing waits for the device (a CPU vector is copied up first).  The object keeps a private device copy of
        the vector; ``state_dict()``, ``parameters()`` and a later engine rebuild (a larger batch, ``set_gemm_dtype``, ``set_low_latency``,
        ``to``) read the new weights from it.  Without a live engine the values go into the host state and the engine is built on first use.
        Refused before anything is enqueued: a vector of another length, dtype or rank, or on another device than the engine's."""
        if not isinstance(flat, torch.Tensor):
            raise TypeError(f"load_flat: a torch tensor is expected, got {type(flat).__name__}")
        if flat.dim() != 1 or flat.numel() != self.param_count:
            raise ValueError(f"load_flat: a vector of shape {tuple(flat.shape)}; this model's parameters are ({self.param_count},)")
        if flat.dtype != torch.float32:
            raise TypeError(f"load_flat: dtype {flat.dtype}; the flat parameter vector is float32")
        flat = flat.detach()
        if self._engine is None:
            self._state = self._state_from_flat(flat.cpu())
            self._flat = None
            return self
        dev = self._engine_device
        if flat.device.type != "cpu" and (flat.device.type != "cuda" or flat.device.index != dev.index):
            raise ValueError(f"load_flat: the vector is on {flat.device}, the engine on {dev}")
        with torch.cuda.device(dev):
            if self._flat is None or self._flat.device != dev:
                self._flat = torch.empty(self.param_count, dtype=torch.float32, device=dev)
            self._flat.copy_(flat)                  # (stream-ordered: the caller may overwrite its vector right after this call)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _lib.check(_lib.lib().tld_engine_refresh_weights(self._engine, C.c_void_p(self._flat.data_ptr()), self.param_count, C.c_void_p(stream)),
                       "tld_engine_refresh_weights")
        self._flat_stale = True
        return self

    # ---- engine management ---------------------------------------------------------------------------
    def _drop_engine(self):
        if self._session is not None:                        # (the engine goes, and its session with it)
            self._session.close()
        if self._engine is not None:
            _lib.lib().tld_engine_destroy(self._engine)       # (the C ABI restores the caller's current device)
        self._engine = None
        self._engine_batch = 0

    def __del__(self):
        try:
            self._drop_engine()
        except Exception:
            pass

    def _resolve_device(self, t: Optional[torch.Tensor] = None) -> torch.device:
        dev = t.device if t is not None else self._device
        if dev is None or dev.type != "cuda":
            raise RuntimeError("Denoiser runs on a HIP device only (tensor/device is %r); there is no CPU path" % (dev,))
        if not torch.cuda.is_available():
            raise RuntimeError("no HIP device visible to PyTorch; the engine cannot run")
        return torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())

    def _ensure_engine(self, model_batch: int, dev: torch.device):
        if self._engine is not None and self._engine_batch >= model_batch and self._engine_device == dev:
            return self._engine
        if self._session is not None and not self._session.closed:
            raise RuntimeError(f"a sampler session is open on this model's engine (capacity {self._engine_batch} model samples): a call that needs a new "
                               f"engine ({model_batch} on {dev}) would destroy it; close the session first")
        self._drop_engine()
        L = _lib.lib()
        cap = model_batch if self._low_latency else max(model_batch, 8)       # (the low-latency class is bounded by capacity: no head-room there)
        cfg = _lib.TldConfig(self.image_size, self.noise_embed_dims, self.patch_size, self.embed_dim, self.n_layers,
                             self.text_emb_size, self.n_channels, self.mlp_multiplier, cap, dev.index)
        h = C.c_void_p()
        _lib.check(L.tld_engine_create(C.byref(cfg), C.byref(h)), "tld_engine_create")
        self._engine_skip = self._env_guidance_skip()
        try:
            if self._gemm_dtype:
                _lib.check(L.tld_engine_set_gemm_dtype(h, self._gemm_dtype), "tld_engine_set_gemm_dtype")
            if self._low_latency:
                _lib.check(L.tld_engine_set_low_latency(h, int(self._low_latency)), "tld_engine_set_low_latency")
            for k, t in self._state.items():
                if t.dtype == torch.int64:
                    continue
                a = t.contiguous()
                shape = (C.c_int64 * a.dim())(*a.shape)
                _lib.check(L.tld_engine_load_tensor(h, k.encode(), C.c_void_p(a.data_ptr()), shape, a.dim(),
                                                    _lib.DTYPE_F32), f"tld_engine_load_tensor({k})")
            _lib.check(L.tld_engine_finalize_weights(h), "tld_engine_finalize_weights")
        except Exception:
            L.tld_engine_destroy(h)
            raise
        self._engine, self._engine_batch, self._engine_device = h, cap, dev
        return h

    @staticmethod
    def _env_guidance_skip() -> bool:
        """``TLD_GUIDANCE_SKIP`` as ``tld_engine_create`` reads it (atoi: unset = on, anything but a non-zero integer = off)."""
        v = os.environ.get("TLD_GUIDANCE_SKIP")
        if v is None:
            return True
        try:
            return int(v.strip()) != 0
        except ValueError:
            return False

    def set_gemm_dtype(self, name: str) -> "Denoiser":
        """Operand type of the QKV / MLP GEMMs: ``"bf16"`` (default) or ``"fp8"`` (MX-fp8: e4m3 elements, E8M0 scale
        per 32 K-elements, activations quantised on the fly; BASELINE config C4 -- not a mode of the reference)."""
        code = {"bf16": 0, "fp8": 1}[name]
        if code != self._gemm_dtype:
            self._drop_engine()
        self._gemm_dtype = code
        return self

    LOW_LATENCY_MAX_ROWS = 4096          # engine capacity (model batch x tokens) of the low-latency class: kLowLatMaxRows in csrc/tld_engine.hip

    LOW_LATENCY_MAX_ROWS_SINGLE = 1024   # ... of class 2 (eight K-splits): kLowLatMaxRows2

    def set_low_latency(self, on=True) -> "Denoiser":
        """Serve SMALL batches in a low-latency capacity class (``tld_engine_set_low_latency``): the MLP down projection of every block runs as
        split-K, which cuts a one-image 35-step ``generate`` from ~37 ms to ~31 ms (``True`` / ``1``: four K-splits, up to ``LOW_LATENCY_MAX_ROWS``
        token rows = 8 images at 256 px) or ~30 ms (``2``: eight K-splits, up to ``LOW_LATENCY_MAX_ROWS_SINGLE`` = one or two images per call --
        the reference's serving pattern, one prompt per call, tld/app.py:48-65).  A class is a property of this model object, not of a call: every
        engine it builds is in the class, results inside it are bit-identical across batch sizes, and they differ from the default class (and from
        the other class) only in the fp32 summation order of that product.  A batch whose CFG-doubled size x tokens exceeds the class's capacity
        raises -- build a second model object for bulk generation."""
        on = int(on)
        if on not in (0, 1, 2):
            raise ValueError("set_low_latency: False / 0 (default class), True / 1 (four K-splits) or 2 (eight K-splits, one or two images per call)")
        if on != self._low_latency:
            self._drop_engine()
        self._low_latency = on
        return self

    def reserve(self, model_batch: int, device=None) -> "Denoiser":
        """Build the engine for up to ``model_batch`` samples per forward (CFG-doubled count)."""
        if device is not None:
            self.to(device)
        self._ensure_engine(model_batch, self._resolve_device())
        return self

    # ---- the call contract ----------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, x: torch.Tensor, noise_level: torch.Tensor, label: torch.Tensor) -> torch.Tensor:
        dev = self._resolve_device(x)
        if x.dim() != 4 or x.shape[1] != self.n_channels or x.shape[2] != self.image_size or x.shape[3] != self.image_size:
            raise RuntimeError(f"expected x of shape [B,{self.n_channels},{self.image_size},{self.image_size}], got {tuple(x.shape)}")
        B = x.shape[0]
        if B == 0:                                   # empty batch: nothing to enqueue (nn.Module would return an empty tensor)
            return torch.empty_like(x)
        if noise_level.numel() != B or label.shape != (B, self.text_emb_size):
            raise RuntimeError(f"noise_level {tuple(noise_level.shape)} / label {tuple(label.shape)} do not match batch {B}")
        dt = x.dtype
        if dt not in _IO_DTYPES:
            raise TypeError(f"unsupported tensor dtype {dt}")
        h = self._ensure_engine(B, dev)
        xc = x.contiguous()
        nc = noise_level.to(device=dev, dtype=dt).contiguous()
        lc = label.to(device=dev, dtype=dt).contiguous()
        out = torch.empty_like(xc)
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().tld_denoiser_forward(h, xc.data_ptr(), nc.data_ptr(), lc.data_ptr(), out.data_ptr(),
                                                       B, _IO_DTYPES[dt], C.c_void_p(stream)), "tld_denoiser_forward")
        return out

    __call__ = forward

    @torch.no_grad()
    def sample_latents(self, x_T: torch.Tensor, labels: torch.Tensor, coeffs: np.ndarray, class_guidance: float,
                       sharp_f: float = 0.0, bright_f: float = 0.0, trace: bool = False):
        """On-device CFG sampler (tld_sample): x_T [B,C,S,S], labels [B,text] (conditional half only),
        coeffs = schedule.step_coefficients(...).  Returns fp32 latent [B,C,S,S] (+ traces)."""
        co = np.ascontiguousarray(coeffs, dtype=np.float32)
        return self._run_sampler(x_T, labels, co.shape[0], trace, lambda h, B, eps, z0, m, lab, neg, out, tx0, txt, stream: _lib.check(
            _lib.lib().tld_sample(h, eps, lab, co.ctypes.data_as(C.POINTER(C.c_float)), co.shape[0], float(class_guidance), float(sharp_f),
                                  float(bright_f), out, B, tx0, txt, stream), "tld_sample"))

    def _run_sampler(self, noise, labels, n_levels: int, trace: bool, call, init_latents=None, mask=None, neg_labels=None, order=None,
                     new_trace=torch.empty, model_batch=None):
        """What the three sampler entries share around their C call: the device, the ``init_latents`` / ``mask`` shape checks, the empty
        batch, the engine for the CFG-doubled batch (or ``model_batch(engine_skip)``, a guided call's own largest step), the operands as contiguous fp32 on the device (rows gathered in ``order`` when the
        engine wants its own), the result and -- with ``trace`` -- the [n_levels-1,B,C,S,S] trace tensors from ``new_trace``, then
        ``call(engine, B, noise, init_latents, mask, labels, neg_labels, out, trace_x0, trace_xt, stream)`` -- pointers, NULL for an absent
        operand -- under the device context on its current stream.  Results come back in the caller's order."""
        dev = self._resolve_device(noise)
        B = noise.shape[0]
        if init_latents is not None and tuple(init_latents.shape) != tuple(noise.shape):
            raise ValueError(f"init_latents {tuple(init_latents.shape)} != noise {tuple(noise.shape)}")
        if mask is not None and tuple(mask.shape) != (B, 1) + tuple(noise.shape[2:]):
            raise ValueError(f"mask {tuple(mask.shape)}: expected {(B, 1) + tuple(noise.shape[2:])}")
        if B == 0:
            z = torch.empty_like(noise, dtype=torch.float32)
            return (z, None, None) if trace else z
        if model_batch is None:
            h = self._ensure_engine(2 * B, dev)
        else:       # the engine at hand decides with its own TLD_GUIDANCE_SKIP where it is large enough; a new one reads the environment now
            need = model_batch(self._engine_skip)
            if self._engine is None or self._engine_batch < need or self._engine_device != dev:
                need = model_batch(self._env_guidance_skip())
            h = self._ensure_engine(need, dev)
        idx = None if order is None else torch.tensor(order, device=dev)

        def operand(t):
            if t is None:
                return None
            t = t.to(device=dev, dtype=torch.float32)
            return (t if idx is None else t[idx]).contiguous()

        eps, z0, m, lab, neg = operand(noise), operand(init_latents), operand(mask), operand(labels), operand(neg_labels)
        out = torch.empty_like(eps)
        tx0 = txt = None
        if trace:
            tx0 = new_trace((n_levels - 1,) + tuple(eps.shape), device=dev, dtype=torch.float32)
            txt = new_trace(tx0.shape, device=dev, dtype=torch.float32)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        with torch.cuda.device(dev):
            call(h, B, ptr(eps), ptr(z0), ptr(m), ptr(lab), ptr(neg), ptr(out), ptr(tx0), ptr(txt),
                 C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if idx is not None:
            inv = torch.empty_like(idx)
            inv[idx] = torch.arange(B, device=dev)
            out = out[inv]
            if trace:
                tx0, txt = tx0[:, inv], txt[:, inv]
        return (out, tx0, txt) if trace else out

    @torch.no_grad()
    def sample_latents_from(self, noise: torch.Tensor, init_latents: torch.Tensor, labels: torch.Tensor, coeffs: np.ndarray,
                            class_guidance: float, start_mix: float, mask: Optional[torch.Tensor] = None, sharp_f: float = 0.0,
                            bright_f: float = 0.0, trace: bool = False):
        """On-device CFG sampler for image-to-image and inpainting (tld_sample_from): the trajectory starts at
        ``start_mix * noise + (1 - start_mix) * init_latents`` (``start_mix = 1.0``: at ``noise`` itself) and runs the levels of ``coeffs``
        (the remaining ones, ``schedule.truncate_levels``); with ``mask`` [B,1,S,S] in [0,1] (1 = regenerate) the kept region is re-imposed
        after every step and on the final prediction.  Returns fp32 latent [B,C,S,S] (+ traces)."""
        co = np.ascontiguousarray(coeffs, dtype=np.float32)
        return self._run_sampler(noise, labels, co.shape[0], trace, lambda h, B, eps, z0, m, lab, neg, out, tx0, txt, stream: _lib.check(
            _lib.lib().tld_sample_from(h, eps, z0, m, float(start_mix), lab, co.ctypes.data_as(C.POINTER(C.c_float)), co.shape[0],
                                       float(class_guidance), float(sharp_f), float(bright_f), out, B, tx0, txt, stream), "tld_sample_from"),
            init_latents=init_latents, mask=mask)

    @torch.no_grad()
    def sample_latents_requests(self, noise: torch.Tensor, labels: torch.Tensor, coeff_list, guidance, *, neg_labels=None, init_latents=None,
                                start_mix=None, mask=None, sharp_f: float = 0.0, bright_f: float = 0.0, trace: bool = False, guidance_steps=None,
                                noise_coeffs=None, noise_keys=None, shape=None):
        """B independent requests in one on-device sampler call (tld_sample_requests).

        ``noise`` [B,C,S,S], ``labels`` [B,text]; ``coeff_list``: B tables ``schedule.step_coefficients(...)`` (each request's own levels
        and number of them); ``guidance``: B scales.  ``neg_labels``: None, a [B,text] tensor, or a length-B sequence of [text] tensors /
        None (a request without one keeps the zero label).  ``init_latents`` [B,C,S,S] + ``start_mix`` (B values in (0, 1], default 1) +
        ``mask`` [B,1,S,S] as in ``sample_latents_from``; a text-to-image request in a call that carries masks takes an all-ones mask.
        Request b's result equals, bit for bit, ``sample_latents`` / ``sample_latents_from`` of that request alone.  Returns fp32 latents
        [B,C,S,S] in the caller's order; with ``trace`` also [n_max-1,B,C,S,S] predictions and states, zero where a request had finished.
        ``guidance_steps``: B arrays, request b's guidance per forward (``coeff_list[b].shape[0]`` values, e.g. ``schedule.guidance_table``); the
        call is then tld_sample_requests_guided: ``guidance`` is ignored (it may be None), a forward whose value is exactly
        1.0 runs no unconditional sample, and the engine is reserved for the largest step, ``max_i (B_i + U_i)`` samples, instead of 2 B.
        ``noise_coeffs`` + ``noise_keys`` (both or neither): the call is tld_sample_requests_stochastic.  ``noise_coeffs``: B
        arrays, request b's ``e`` per forward (``coeff_list[b].shape[0]`` values, finite, >= 0, the last one 0 -- the second result of
        ``schedule.step_coefficients(..., eta)``, whose table belongs in ``coeff_list``); ``noise_keys``: B ints, each request's 64-bit noise key
        (``schedule.noise_key``).  After an inner step's update the kernel adds ``e z``, z the normals of (key, forward, element): request b's
        result is bit for bit that of the request alone with the same key, and all-zero arrays give the call without them.  With
        ``guidance_steps`` the model batches are the guided call's; without, the CFG-doubled ones.
        ``shape``: B rows ``(eta_par, norm_r, beta, phi)`` (``schedule.check_guidance_shape``); the call is then tld_sample_requests_shaped
        (DESIGN.md section 7.16), with or without any of the above: guidance rescale and adaptive projected guidance on the requests whose row is
        not ``schedule.GUIDANCE_SHAPE_NEUTRAL``.  A neutral row is the request without ``shape``, bit for bit, and request b still equals the
        request alone.
        Its own here: the records' checks, the engine's order, the row cap and the negative labels as one tensor; the rest is ``_run_sampler``."""
        from . import schedule
        B = noise.shape[0]
        if noise.dim() != 4 or tuple(noise.shape[1:]) != (self.n_channels, self.image_size, self.image_size):
            raise ValueError(f"noise {tuple(noise.shape)}: expected [B,{self.n_channels},{self.image_size},{self.image_size}]")
        if tuple(labels.shape) != (B, self.text_emb_size):
            raise ValueError(f"labels {tuple(labels.shape)}: expected {(B, self.text_emb_size)}")
        tabs = [np.ascontiguousarray(c, dtype=np.float32) for c in coeff_list]
        steps = None
        if guidance_steps is not None:
            steps = [np.ascontiguousarray(t, dtype=np.float32) for t in guidance_steps]
            if len(steps) != B:
                raise ValueError(f"guidance_steps: {len(steps)} entries for {B} requests")
            guidance = [1.0] * B
        guid = [float(g) for g in guidance]
        mix = [1.0] * B if start_mix is None else [float(v) for v in start_mix]
        for what, seq in (("coeff_list", tabs), ("guidance", guid), ("start_mix", mix)):
            if len(seq) != B:
                raise ValueError(f"{what}: {len(seq)} entries for {B} requests")
        for b, t in enumerate(tabs):
            if t.ndim != 2 or t.shape[1] != 6 or t.shape[0] < 2:
                raise ValueError(f"coeff_list[{b}] {t.shape}: expected [n_levels >= 2, 6]")
            if not np.isfinite(guid[b]):
                raise ValueError(f"guidance[{b}] = {guid[b]} is not finite")
            if not (0.0 < mix[b] <= 1.0):
                raise ValueError(f"start_mix[{b}] = {mix[b]} outside (0, 1]")
            if steps is not None and (steps[b].ndim != 1 or steps[b].shape[0] != t.shape[0]):
                raise ValueError(f"guidance_steps[{b}] {steps[b].shape}: expected [{t.shape[0]}], one value per forward")
            if steps is not None and not np.isfinite(steps[b]).all():
                raise ValueError(f"guidance_steps[{b}] holds a value that is not finite")
        if init_latents is None and (mask is not None or any(v < 1.0 for v in mix)):
            raise ValueError("init_latents is required with a mask or with a start_mix < 1")
        if (noise_coeffs is None) != (noise_keys is None):
            raise ValueError("noise_coeffs and noise_keys come together")
        ecs = keys = None
        if noise_coeffs is not None:
            ecs = [np.ascontiguousarray(t, dtype=np.float32) for t in noise_coeffs]
            keys = [int(k) for k in noise_keys]
            for what, seq in (("noise_coeffs", ecs), ("noise_keys", keys)):
                if len(seq) != B:
                    raise ValueError(f"{what}: {len(seq)} entries for {B} requests")
            for b, t in enumerate(ecs):
                if t.ndim != 1 or t.shape[0] != tabs[b].shape[0]:
                    raise ValueError(f"noise_coeffs[{b}] {t.shape}: expected [{tabs[b].shape[0]}], one value per forward")
                if not (np.isfinite(t).all() and (t >= 0).all()):
                    raise ValueError(f"noise_coeffs[{b}] holds a value that is not finite and >= 0")
                if t[-1] != 0:
                    raise ValueError(f"noise_coeffs[{b}][-1] = {t[-1]}: the final prediction takes no noise, expected 0")
                if not 0 <= keys[b] < 1 << 64:
                    raise ValueError(f"noise_keys[{b}] = {keys[b]}: expected a 64-bit unsigned value")
        shp = None
        if shape is not None:
            rows = [tuple(r) for r in shape]
            if len(rows) != B:
                raise ValueError(f"shape: {len(rows)} entries for {B} requests")
            for b, r in enumerate(rows):
                if len(r) != 4:
                    raise ValueError(f"shape[{b}] has {len(r)} values: expected (eta_par, norm_r, beta, phi)")
            shp = [schedule.check_guidance_shape(r[3], r[0], r[1], r[2]) for r in rows]
        neg, has_neg = None, [False] * B
        if neg_labels is not None:
            if isinstance(neg_labels, torch.Tensor):
                if tuple(neg_labels.shape) != (B, self.text_emb_size):
                    raise ValueError(f"neg_labels {tuple(neg_labels.shape)}: expected {(B, self.text_emb_size)}")
                neg, has_neg = neg_labels, [True] * B
            else:
                rows = list(neg_labels)
                if len(rows) != B:
                    raise ValueError(f"neg_labels: {len(rows)} entries for {B} requests")
                for b, r in enumerate(rows):
                    if r is not None and tuple(r.shape) != (self.text_emb_size,):
                        raise ValueError(f"neg_labels[{b}] {tuple(r.shape)}: expected {(self.text_emb_size,)}")
                has_neg = [r is not None for r in rows]
                if any(has_neg):
                    dev = self._resolve_device(noise)
                    neg = torch.stack([torch.zeros(self.text_emb_size, device=dev) if r is None else r.detach().to(dev, torch.float32) for r in rows])
        counts = [t.shape[0] for t in tabs]
        order = schedule.request_order(counts)                  # the engine wants non-increasing level counts: _run_sampler gathers and un-sorts
        n_max = counts[order[0]] if B else 0
        rows_needed = schedule.request_cond_rows([tabs[b] for b in order], sum(has_neg)) if B else 0
        if rows_needed > schedule.REQUEST_ROW_CAP:
            raise ValueError(f"the call needs {rows_needed} conditioning rows (distinct noise levels + labels): at most {schedule.REQUEST_ROW_CAP}")
        table = np.zeros((B, n_max, 6), dtype=np.float32)
        recs = (_lib.TldSampleRequest * B)()
        for k, b in enumerate(order):
            table[k, :counts[b]] = tabs[b]
            recs[k] = _lib.TldSampleRequest(counts[b], guid[b], mix[b], int(has_neg[b]))
        gtab, model_batch = None, None
        if steps is not None:
            gtab = np.zeros((B, n_max), dtype=np.float32)
            for k, b in enumerate(order):
                gtab[k, :counts[b]] = steps[b]

            def model_batch(skip):       # the largest step of the plan the engine makes (csrc/tld_sample_plan.h; held against it on the CPU)
                if not B:
                    return 0
                sc = [counts[b] for b in order]
                U = schedule.guided_rows(sc, [steps[b] for b in order], skip)[0]
                return max(bi + u for bi, u in zip(schedule.active_prefix(sc), U))

        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        # traces start as zeros: the engine leaves a finished request's slots alone
        common = dict(init_latents=init_latents, mask=mask, neg_labels=neg, order=order, new_trace=torch.zeros)
        etab = ktab = None
        if ecs is not None:
            etab = np.zeros((B, n_max), dtype=np.float32)
            ktab = np.zeros(B, dtype=np.uint64)
            for k, b in enumerate(order):
                etab[k, :counts[b]] = ecs[b]
                ktab[k] = keys[b]
        kp = None if ktab is None else ktab.ctypes.data_as(C.POINTER(C.c_uint64))
        # the entry and what it takes between the coefficient table and n_max
        if shp is not None:              # (noise_coeff / noise_keys NULL: no noise; guidance NULL: as in the stochastic entry)
            stab = np.ascontiguousarray([shp[b] for b in order], dtype=np.float32).reshape(B, 4)
            entry, extra = "tld_sample_requests_shaped", (fp(gtab), fp(etab), kp, fp(stab))
        elif ecs is not None:            # (guidance NULL: the records' scales on the CFG-doubled batch)
            entry, extra = "tld_sample_requests_stochastic", (fp(gtab), fp(etab), kp)
        elif steps is not None:
            entry, extra = "tld_sample_requests_guided", (fp(gtab),)
        else:
            entry, extra = "tld_sample_requests", ()
        return self._run_sampler(noise, labels, n_max, trace, lambda h, B, eps, z0, m, lab, ng, out, tx0, txt, stream: _lib.check(
            getattr(_lib.lib(), entry)(h, eps, z0, m, lab, ng, recs, fp(table), *extra, n_max, float(sharp_f), float(bright_f), out, B, tx0, txt, stream),
            entry), model_batch=model_batch, **common)

    def open_session(self, slots: int, cond_rows: Optional[int] = None, sharp_f: float = 0.0, bright_f: float = 0.0, device=None) -> "DenoiserSession":
        """A sampler session on this model's engine (``tld_session_open``), the raw form: ``slots`` requests run at once, each
        at its own level, and requests are admitted between steps.  ``cond_rows``: the session's conditioning-row table (the zero row, one or
        two label rows per live request and one shared row per distinct noise level); default ``min(1024, 1 + slots * 66)``, room for ``slots``
        requests of 64 levels on distinct schedules.  The engine is reserved for ``2 * slots`` model samples.  One session per model at a time; while
        it is open the other calls of this model raise (``TLD_ERR_STATE``)."""
        if self._session is not None and not self._session.closed:
            raise RuntimeError("a sampler session is already open on this model: one session per engine")
        slots = int(slots)
        if slots < 1:
            raise ValueError(f"open_session: slots = {slots}: at least one")
        if device is not None:
            self.to(device)
        dev = self._resolve_device()
        rows = min(1024, 1 + slots * 66) if cond_rows is None else int(cond_rows)
        h = self._ensure_engine(2 * slots, dev)
        out = C.c_void_p()
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            _lib.check(_lib.lib().tld_session_open(h, slots, rows, float(sharp_f), float(bright_f), C.c_void_p(stream.cuda_stream), C.byref(out)),
                       "tld_session_open")
        self._session = DenoiserSession(self, out, slots, rows, dev)
        return self._session

    # ---- test / bench hooks -----------------------------------------------------------------------------
    # launch paths of tld_engine_debug_paths, by bit number (include/tld_hip.h; None: a bit no default engine sets).  "tail folded" (out_proj folded into
    # the last block's down projection) comes with the tail_mfma<NT> bit of its patch-feature tiles.  Bit 49, the VALU tail of widths that are no multiple
    # of 128, is set only with TLD_FOLD_TAIL=0 since the fold (tests/test_gpu_tail_fold.py holds it there): the folded tail takes every width.
    PATH_NAMES = ("embed plain", "embed_mfma<2>", "embed_mfma<4>", "embed_mfma<6>", "embed_mfma<8>", "layernorm q4<1>", "layernorm q4<2>", "layernorm q4<3>",
                  "layernorm q4<4>", "layernorm generic", "layernorm mx8", "QKV fused with attention", "QKV LayerNorm-1 fold", "QKV plain", "attention 256",
                  "attention chunked", "tail folded", "attention 64", None, "attention masked", "cross_row_mfma<1>", "cross_row_mfma<2>",
                  "cross_row_mfma<3>", "cross_row_mfma<4>", "cross_row gpw 1", "cross_row gpw > 1", "cross_row VALU", "cross_row x_in fan-out",
                  "up fused 16", "up fused 32 + seam", "up fused 16 4-wave", "up alone", "depthwise whole image", "depthwise tiled", "depthwise streaming",
                  "down with stats_out", "down without stats_out", "down 8-wave", "down 4-wave 64", "down 4-wave 128", "split-K x4", "split-K x8",
                  "split-K 4-wave", "split-K finisher<12>", "split-K finisher<6>", "tail_mfma<1>", "tail_mfma<2>", "tail_mfma<3>", "tail_mfma<4>", None,
                  "update", "update_from", "update_from masked", "start_mix")
    # the writers of the MX-fp8 A operand, by bit number (bit 10 is in PATH_NAMES too): held by tests/test_gpu_fp8_stages.py
    FP8_PATH_NAMES = {10: "layernorm mx8", 54: "fp8 separate quantisation pass", 55: "fp8 cross_row writer", 56: "fp8 depthwise tiled",
                      57: "fp8 depthwise streaming"}

    # the two-head form of the fused QKV + attention kernel (taken where whole rounds of head pairs fill the device, or under TLD_QKV_ATTN_PAIR=2): not in
    # PATH_NAMES, whose cases are small batches; held by tests/test_gpu_qkv_pair.py
    QKV_PAIR_PATH_NAMES = {61: "QKV + attention, two heads per tile"}

    # the launch paths of sample_latents_requests, by bit number
    SAMPLER_PATH_NAMES = {58: "update_requests", 59: "update_requests masked", 60: "start_mix per request"}
    # ... and of a sampler session's step
    SESSION_PATH_NAMES = {62: "update_session"}

    def sample_rows(self):
        """``(cond, uncond)``: the model samples the last sampler call on this model's engine enqueued (``tld_engine_sample_rows``); the CFG-doubled
        entries report ``sum(n_levels)`` twice, a guided call ``sum(n_levels)`` and the unconditional samples it did run."""
        c, u = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().tld_engine_sample_rows(self._engine, C.byref(c), C.byref(u)), "tld_engine_sample_rows")
        return int(c.value), int(u.value)

    def set_debug(self, enable: bool = True):
        """Stage capture of the forward (``tld_engine_set_debug``): allocates (frees) the snapshot memory of the current engine."""
        _lib.check(_lib.lib().tld_engine_set_debug(self._engine, int(enable)), "tld_engine_set_debug")

    def set_debug_step(self, step: int):
        """Sampler step whose stages a debug ``sample_latents`` keeps (negative: every step, so the last one remains)."""
        _lib.check(_lib.lib().tld_engine_set_debug_step(self._engine, int(step)), "tld_engine_set_debug_step")

    def debug_paths(self) -> int:
        m = C.c_uint64()
        _lib.check(_lib.lib().tld_engine_debug_paths(self._engine, C.byref(m)), "tld_engine_debug_paths")
        return int(m.value)

    def stage_shape(self, name: str):
        sh = (C.c_int64 * 4)()
        _lib.check(_lib.lib().tld_engine_stage_shape(self._engine, name.encode(), sh), f"tld_engine_stage_shape({name})")
        sh = list(sh)
        while len(sh) > 1 and sh[-1] == 1:
            sh.pop()
        return tuple(sh)

    def read_stage(self, name: str, shape=None) -> np.ndarray:
        """A captured stage as fp32; ``shape`` defaults to the stage's logical shape, and a shape of another size is refused by the library."""
        out = np.empty(self.stage_shape(name) if shape is None else shape, dtype=np.float32)
        _lib.check(_lib.lib().tld_engine_read_stage(self._engine, name.encode(),
                                                    out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                   f"tld_engine_read_stage({name})")
        return out

    def set_profile(self, classes=()):
        mask = 0
        for c in classes:
            mask |= 1 << _lib.KERNEL_CLASSES.index(c)
        _lib.check(_lib.lib().tld_engine_set_profile(self._engine, mask), "tld_engine_set_profile")

    def reserve_profile(self, cls: str, launches: int):
        """Pre-create the event pairs ``launches`` timed launches of class ``cls`` will record into."""
        _lib.check(_lib.lib().tld_engine_profile_reserve(self._engine, _lib.KERNEL_CLASSES.index(cls), int(launches)),
                   "tld_engine_profile_reserve")

    def get_profile(self, cls: str):
        ms, n = C.c_double(), C.c_int64()
        _lib.check(_lib.lib().tld_engine_get_profile(self._engine, _lib.KERNEL_CLASSES.index(cls), C.byref(ms),
                                                     C.byref(n)), "tld_engine_get_profile")
        return ms.value, n.value


class DenoiserSession:
    """A sampler session on a ``Denoiser``'s engine (``Denoiser.open_session``; ``tld_session_*``), the raw form: slots,
    tables and device tensors.  ``DiffusionGenerator.open_session`` builds requests the way the ``generate_latents*`` calls do.  A context manager;
    every call runs on the stream that was current at ``open_session`` and raises on another one."""

    def __init__(self, model: Denoiser, handle, slots: int, cond_rows: int, dev: torch.device):
        self.model, self._h, self.slots, self.cond_rows, self.device = model, handle, slots, cond_rows, dev
        self.closed = False
        self._keep = {}                   # slot -> the device tensors of the request in it (they must outlive the copies admit enqueues)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _open(self):
        if self.closed:
            raise RuntimeError("the sampler session is closed")

    @torch.no_grad()
    def admit(self, noise: torch.Tensor, label: torch.Tensor, coeffs, guidance: float = 3.0, *, neg_label=None, guidance_steps=None, noise_coeff=None,
              noise_key=None):
        """One request into a free slot (``tld_session_admit``): ``noise`` [C,S,S] (or [1,C,S,S]), ``label`` [text], ``coeffs`` its table
        ``schedule.step_coefficients(...)``, ``guidance`` its scale or ``guidance_steps`` one value per forward, ``neg_label`` [text] or None,
        ``noise_coeff`` + ``noise_key`` (both or neither) as in ``sample_latents_requests``.  Returns the slot, or None when the session has no
        room now (no free slot, or too few free conditioning rows): ask again after a ``step``."""
        self._open()
        m = self.model
        want = (m.n_channels, m.image_size, m.image_size)
        if tuple(noise.shape) == (1,) + want:
            noise = noise[0]
        if tuple(noise.shape) != want:
            raise ValueError(f"noise {tuple(noise.shape)}: expected {want}")
        if tuple(label.shape) == (1, m.text_emb_size):
            label = label[0]
        if tuple(label.shape) != (m.text_emb_size,):
            raise ValueError(f"label {tuple(label.shape)}: expected {(m.text_emb_size,)}")
        if neg_label is not None and tuple(neg_label.shape) != (m.text_emb_size,):
            raise ValueError(f"neg_label {tuple(neg_label.shape)}: expected {(m.text_emb_size,)}")
        co = np.ascontiguousarray(coeffs, dtype=np.float32)
        if co.ndim != 2 or co.shape[1] != 6 or co.shape[0] < 2:
            raise ValueError(f"coeffs {co.shape}: expected [n_levels >= 2, 6]")
        n = co.shape[0]
        if (noise_coeff is None) != (noise_key is None):
            raise ValueError("noise_coeff and noise_key come together")
        fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        gs = ec = None
        if guidance_steps is not None:
            gs = np.ascontiguousarray(guidance_steps, dtype=np.float32)
            if gs.shape != (n,):
                raise ValueError(f"guidance_steps {gs.shape}: expected [{n}], one value per forward")
        if noise_coeff is not None:
            ec = np.ascontiguousarray(noise_coeff, dtype=np.float32)
            if ec.shape != (n,):
                raise ValueError(f"noise_coeff {ec.shape}: expected [{n}], one value per forward")
            if not 0 <= int(noise_key) < 1 << 64:
                raise ValueError(f"noise_key = {noise_key}: expected a 64-bit unsigned value")
        key = None if noise_key is None else C.c_uint64(int(noise_key))
        dev = self.device
        t = lambda x: None if x is None else x.detach().to(device=dev, dtype=torch.float32).contiguous()
        eps, lab, neg = t(noise), t(label), t(neg_label)
        ptr = lambda x: C.c_void_p(None if x is None else x.data_ptr())
        rq = _lib.TldSessionRequest(n, float(1.0 if gs is not None else guidance), int(neg is not None), 0, fp(co), fp(gs), fp(ec),
                                    None if key is None else C.pointer(key), ptr(eps), ptr(lab), ptr(neg))
        slot = C.c_int32(-1)
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().tld_session_admit(self._h, C.byref(rq), self._stream(), C.byref(slot)), "tld_session_admit")
        if slot.value < 0:
            return None
        self._keep[slot.value] = (eps, lab, neg)
        return int(slot.value)

    @torch.no_grad()
    def step(self):
        """One model forward for every live request, each at its own level, and one elementwise update (``tld_session_step``); returns the slots
        whose request ran its final forward (ascending).  With no live request nothing is enqueued."""
        self._open()
        done, n = (C.c_int32 * self.slots)(), C.c_int32(0)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_session_step(self._h, self._stream(), done, self.slots, C.byref(n)), "tld_session_step")
        return [int(done[k]) for k in range(n.value)]

    @torch.no_grad()
    def latent(self, slot: int) -> torch.Tensor:
        """A copy [C,S,S] of the slot's result, enqueued on the session's stream: the latent of the request that last finished in it."""
        self._open()
        m = self.model
        out = torch.empty(m.n_channels, m.image_size, m.image_size, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().tld_session_copy_latent(self._h, int(slot), C.c_void_p(out.data_ptr()), self._stream()), "tld_session_copy_latent")
        return out

    def stats(self) -> dict:
        self._open()
        v = (C.c_int64 * 5)()
        _lib.check(_lib.lib().tld_session_stats(self._h, v), "tld_session_stats")
        return dict(live=int(v[0]), steps=int(v[1]), rows_cond=int(v[2]), rows_uncond=int(v[3]), cond_rows_used=int(v[4]))

    @property
    def live(self) -> int:
        return self.stats()["live"]

    def close(self):
        if self.closed:
            return
        self.closed = True
        _lib.lib().tld_session_close(self._h)
        self._keep.clear()
        if self.model._session is self:
            self.model._session = None

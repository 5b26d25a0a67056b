/*
 * tld_hip.h -- C ABI of libtld_hip.so: the MI355X (gfx950) denoising engine.
 *
 * The reference has no FFI/plugin interface; its boundary is the Python nn.Module call contract
 * between the sampler and the model.  Each entry point below names the
 * reference interface it replaces (paths relative to the reference checkout).  Signatures use plain
 * pointers and sizes only (no torch types): device buffers belong to the caller (PyTorch), packed
 * weights and workspace belong to the engine.  All kernels are enqueued on the caller's HIP stream
 * with no hidden synchronisation.  Every function returns 0 on success or a non-zero status;
 * tld_last_error() returns the thread-local message.  Nothing throws across this boundary.
 */
#ifndef TLD_HIP_H
#define TLD_HIP_H

#include <stdint.h>

#if defined(__GNUC__)
#define TLD_API __attribute__((visibility("default")))
#else
#define TLD_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tld_engine tld_engine;

/* Mirrors tld/configs.py:21-31 DenoiserConfig (dropout is identity at inference and not carried),
 * plus engine sizing.  Replaces the kwargs of Denoiser.__init__ (tld/denoiser.py:86-97). */
typedef struct tld_config {
    int32_t image_size;       /* image_size / patch_size (the token grid's side) must be a multiple of 4; the reference takes any square
                                 grid (tld/transformer_blocks.py:109) -- tld_engine_create says so when it refuses one */
    int32_t noise_embed_dims; /* even */
    int32_t patch_size;       /* n_channels * patch_size^2 (the patch vector) <= 64 */
    int32_t embed_dim;        /* any multiple of the head width 64 up to 1024: heads = embed_dim / 64 (tld/transformer_blocks.py:126-128);
                                 the training engine (tld_train_*) takes the same widths */
    int32_t n_layers;
    int32_t text_emb_size;
    int32_t n_channels;
    int32_t mlp_multiplier;
    int32_t max_batch;        /* largest model batch (CFG-doubled) a forward will see */
    int32_t device_id;        /* HIP device ordinal */
} tld_config;

enum { TLD_DTYPE_F32 = 0, TLD_DTYPE_BF16 = 1, TLD_DTYPE_F16 = 2 };

enum {
    TLD_OK = 0,
    TLD_ERR_INVALID = 1,      /* bad argument / unsupported configuration */
    TLD_ERR_KEY = 2,          /* unknown state_dict key */
    TLD_ERR_SHAPE = 3,        /* tensor shape does not match the configuration */
    TLD_ERR_STATE = 4,        /* call order (weights not finalized, missing tensors) */
    TLD_ERR_HIP = 5           /* a HIP runtime call failed */
};

/* Denoiser(**asdict(cfg)) -- tld/denoiser.py:85-114, tld/diffusion.py:145
 * (No entry point changes the calling thread's current HIP device: each one switches to cfg.device_id
 * for its own duration and restores the previous device before returning.) */
TLD_API int tld_engine_create(const tld_config* cfg, tld_engine** out);

/* Denoiser.load_state_dict, one entry at a time -- tld/diffusion.py:152-153.
 * key is the reference state_dict key; host_ptr is contiguous host memory of `dtype`
 * (TLD_DTYPE_F32; int64 buffers such as precomputed_pos_enc are passed with ndim/shape and ignored). */
TLD_API int tld_engine_load_tensor(tld_engine* e, const char* key, const void* host_ptr, const int64_t* shape,
                           int32_t ndim, int32_t dtype);

/* Builds the weight images on the device (bf16 GEMM operands, folded tables): the loaded tensors go up as one temporary fp32 vector and the kernels of
 * tld_engine_refresh_weights fill the images.  Must follow the loads; fails with TLD_ERR_STATE and names a missing key if the state_dict was
 * incomplete, with TLD_ERR_SHAPE where a tensor's element count is not the configuration's. */
TLD_API int tld_engine_finalize_weights(tld_engine* e);

/* Weights from a flat fp32 DEVICE vector, in place.  The vector is in tld_train_param_layout order -- the reference's
 * Denoiser.named_parameters() order, i.e. the state_dict order without the two registered buffers -- so a training engine's `params` or EMA vector of the
 * same configuration is one.  tld_engine_param_count is its length (= tld_train_param_count of a training engine with the same config; known from create on).
 * tld_engine_refresh_weights rebuilds, with kernels enqueued on hip_stream, every weight image this engine holds in its mode (fp32 copies, bf16 casts,
 * hi / lo splits, transposes, depthwise tap packings, the LayerNorm-1 / LayerNorm-3 folds with their column sums and packed rows, the e4m3 images with
 * their E8M0 scales), each with exactly the bits tld_engine_finalize_weights builds from the same values (it runs the same kernels).  It allocates nothing, frees
 * nothing, stages nothing through the host and synchronises neither the stream nor the device; flat_device is read until the stream has passed the
 * call, and calls on this engine enqueued on the same stream afterwards see the new weights.  The pointer tables built at finalize, the activation
 * buffers, the capacity, the GEMM mode, the low-latency class and the debug / profile state stay; angular_speeds is not a parameter and keeps its
 * value; tld_engine_weight_bytes is unchanged.  A capturing stream is not refused (the call only launches kernels), but capture is not part of the tests.
 * Refusals enqueue nothing and leave the weights as they were:
 *   TLD_ERR_STATE  before tld_engine_finalize_weights (the first load goes through tld_engine_load_tensor);
 *   TLD_ERR_SHAPE  numel differs from tld_engine_param_count;
 *   TLD_ERR_INVALID  a null engine or vector. */
TLD_API int64_t tld_engine_param_count(const tld_engine* e);
TLD_API int tld_engine_refresh_weights(tld_engine* e, const float* flat_device, int64_t numel, void* hip_stream);

/* Operand type of the QKV / MLP GEMMs: 0 = bf16 (default), 1 = MX-fp8 (OCP e4m3 elements with one E8M0 scale per 32
 * K-elements, v_mfma_scale_f32_32x32x64_f8f6f4).  Call between tld_engine_create and tld_engine_finalize_weights.
 * Not in the reference (its model_dtype is fp32 / fp16 / bf16, tld/configs.py:33-37): BASELINE config C4. */
TLD_API int tld_engine_set_gemm_dtype(tld_engine* e, int32_t dtype);

/* Low-latency capacity classes (round 5 / 6; no counterpart in the reference, whose serving path -- tld/app.py:48-65 -- runs one prompt per call on whatever
 * kernels PyTorch picks): the MLP down projection of every block runs as K-splits + a finishing kernel.
 *   on = 1: four K-splits, engines of at most 4096 token rows (max_batch x tokens; e.g. 8 images = 16 CFG-doubled samples at 256 px)
 *   on = 2: eight K-splits, engines of at most 1024 token rows (one or two images per CFG call at 256 px -- the one-prompt-per-call pattern)
 *   on = 0: the default class
 * A one-image 35-step generate takes 37 ms in the default class, 31 ms in class 1, 30 ms in class 2; eight images 46 ms in either.  Results of a class differ from
 * the default class (and from the other class) in the fp32 summation order of that product (same tolerances against the reference); a class is chosen by the CALLER for the engine,
 * never by the batch of a call: inside a class results are bit-identical across batch sizes.
 * May be called any time after tld_engine_create; fails (TLD_ERR_INVALID) on larger engines, on widths other than 384 / 768, on hidden widths that do not split
 * into that many multiples of 64, and on engines in the MX-fp8 GEMM mode (bf16 operands only; tld_engine_set_gemm_dtype(fp8) likewise refuses an engine of these classes). */
TLD_API int tld_engine_set_low_latency(tld_engine* e, int32_t on);

/* Denoiser.forward(x, noise_level, label) -- tld/denoiser.py:116-126 (called at tld/diffusion.py:97-101).
 *   x      [batch, C, S, S]     device, io_dtype
 *   noise  [batch, 1]           device, io_dtype
 *   label  [batch, text_emb]    device, io_dtype
 *   out    [batch, C, S, S]     device, io_dtype (may not alias x)
 * Inputs are not modified. */
TLD_API int tld_denoiser_forward(tld_engine* e, const void* x, const void* noise, const void* label, void* out,
                         int32_t batch, int32_t io_dtype, void* hip_stream);

/* DiffusionGenerator.generate minus RNG and VAE decode -- tld/diffusion.py:54-92 with pred_image
 * (:94-103) and apply_classifier_free_guidance (:122-125) fused on device.
 *   x_T     [batch, C, S, S] fp32 device: initial noise (initialize_image, :105-120, done by caller)
 *   labels  [batch, text_emb] fp32 device: conditional embeddings only; the zero "uncond" half of
 *           :61 is implicit
 *   coeffs  [n_levels, 6] fp32 HOST: (sigma, a, b, c, c1, c2) per forward, see
 *           transformer_latent_diffusion_amd/schedule.py (host float64 algebra of :50-57,:72-81)
 *   out_latent [batch, C, S, S] fp32 device: x0_pred incl. sharp_f/bright_f shifts (:88-89)
 *   trace_x0 / trace_xt: optional device buffers [n_levels-1, batch, C, S, S] fp32 (NULL to skip)
 * batch*2 must be <= max_batch.  The call does NOT synchronise the stream: its host-built tables (sigma per level, token-row
 * indices) travel through a pinned staging buffer owned by the engine, and only a later tld_sample on the same engine waits (on
 * an event, long complete by then) before refilling it; all steps are enqueued asynchronously on hip_stream. */
TLD_API int tld_sample(tld_engine* e, const void* x_T, const void* labels, const float* coeffs, int32_t n_levels,
               float class_guidance, float sharp_f, float bright_f, void* out_latent, int32_t batch,
               void* trace_x0, void* trace_xt, void* hip_stream);

/* Image-to-image and inpainting: tld_sample for a trajectory that starts from a latent instead of pure noise.  It replaces what a
 * PyTorch user writes around the loop of tld/diffusion.py:59-92 -- noising an image with the forward process of the training loop
 * (tld/train.py:130, x_s = s eps + (1 - s) x0) before the first step and re-imposing the known region after every step -- which cannot be done
 * from outside here because the loop runs on the device.  The reference itself has no such entry point.
 *   noise       [batch, C, S, S] fp32 device: eps (initialize_image, :105-120, done by caller)
 *   init_latent [batch, C, S, S] fp32 device: z0 in model space (VAE latent / scale_factor, tld/train.py:122); may be NULL when mask is NULL
 *               and start_mix is 1
 *   mask        [batch, 1, S, S] fp32 device in [0, 1], broadcast over channels: 1 = regenerate, 0 = keep; NULL = no mask
 *   start_mix   s0 in (0, 1]: x_start = s0 eps + (1 - s0) z0; exactly 1 = start from eps itself, as tld_sample does
 *   labels, coeffs, n_levels, class_guidance, sharp_f, bright_f, out_latent, batch, trace_x0, trace_xt: as in tld_sample; coeffs holds the
 *               REMAINING levels only (schedule.truncate_levels), so the first step is first-order
 * Every step is tld_sample's (same kernels for the model, the same elementwise step kernel, one launch per step).  With a mask, after the update to level s_next:  x_t <- m x_t + (1 - m) (s_next eps + (1 - s_next) z0),  and on the final prediction
 * x0 <- m x0 + (1 - m) z0 before the shifts; both are exact where m is 0 or 1.  x0 of the multistep history and trace_x0 stay unblended.
 * Without a mask and with start_mix = 1 the result equals tld_sample's bit for bit.
 * noise, init_latent and mask are read by every step: they must stay valid until the enqueued work has run.  Same rules as tld_sample otherwise:
 * batch*2 <= max_batch, no stream synchronisation, everything is enqueued on hip_stream. */
TLD_API int tld_sample_from(tld_engine* e, const void* noise, const void* init_latent, const void* mask, float start_mix, const void* labels,
               const float* coeffs, int32_t n_levels, float class_guidance, float sharp_f, float bright_f, void* out_latent,
               int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream);

/* B independent requests in ONE sampler call: every request brings its own guidance scale, its own schedule (levels and their number),
 * an optional negative label in place of the zero "uncond" label of tld/diffusion.py:61, and its own image-to-image start.  It replaces what a serving
 * loop around the reference does one call at a time (tld/app.py:48-65, one prompt, one guidance value, one n_iter per call) and cannot be done from
 * outside here because the loop runs on the device.  Request b's result is bit for bit what tld_sample / tld_sample_from return for that request alone.
 *   noise       [batch, C, S, S] fp32 device: eps of every request
 *   init_latent [batch, C, S, S] fp32 device, or NULL when mask is NULL and every start_mix is 1
 *   mask        [batch, 1, S, S] fp32 device in [0, 1] (1 = regenerate), or NULL.  A text-to-image request in a call that carries masks takes an
 *               all-ones mask and any finite init_latent: the blends are then the identity, bit for bit
 *   labels      [batch, text_emb] fp32 device;  neg_labels [batch, text_emb] fp32 device or NULL: row b is read when requests[b].has_negative
 *   requests    HOST array of batch records, ordered by NON-INCREASING n_levels (TLD_ERR_INVALID otherwise; the Python layer sorts and un-sorts)
 *   coeffs      [batch, n_max, 6] fp32 HOST: row b holds schedule.step_coefficients of request b (its REMAINING levels, as in tld_sample_from); entries
 *               past requests[b].n_levels are ignored.  n_max = requests[0].n_levels
 *   sharp_f, bright_f: per call, as in tld_sample
 *   out_latent  [batch, C, S, S] fp32 device; trace_x0 / trace_xt: optional [n_max-1, batch, C, S, S] fp32 device.  Request b fills its first
 *               n_levels[b] - 1 slots; the slots of a request that has already finished are left unwritten
 * All requests start at step 0.  Step i runs the model on the requests with n_levels > i only (a prefix, by the ordering), CFG-doubled: a finished
 * request is not computed again, so the call makes 2 x sum(n_levels) model-sample forwards.  Request b's final step, i = n_levels[b] - 1, writes
 * out_latent[b] (mask blend with init_latent, then the shifts).  The elementwise step is one launch per step of the kernel tld_sample runs; it reads
 * (g, a, b, c, c1, c2, s_next, final) per sample from a device table uploaded once per call.  Conditioning rows: one per DISTINCT float32 sigma of all
 * (request, step) pairs -- requests that share a schedule share rows -- then batch label rows, one zero row and one row per request with has_negative;
 * a call that needs more than 1024 of them is refused (TLD_ERR_INVALID, the count in the message).
 * Same rules as tld_sample otherwise: batch*2 <= max_batch, no stream synchronisation (the host tables travel through the engine's pinned staging
 * buffer), noise / init_latent / mask must stay valid until the enqueued work has run.  Under tld_engine_set_debug(1) the call records its launch paths
 * (bits 58-60) but keeps NO stage; tld_engine_read_stage of a step.* or blk* name after it is "no such stage".  Every refusal happens before anything
 * is enqueued. */
typedef struct tld_sample_request {
    int32_t n_levels;         /* >= 2 */
    float class_guidance;     /* finite */
    float start_mix;          /* in (0, 1]: x_start = s0 eps + (1 - s0) z0; exactly 1 = eps itself (copied, not mixed) */
    int32_t has_negative;     /* != 0: the unconditional half of this request reads neg_labels[b] */
} tld_sample_request;
TLD_API int tld_sample_requests(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels, const void* neg_labels,
               const tld_sample_request* requests, const float* coeffs, int32_t n_max, float sharp_f, float bright_f, void* out_latent,
               int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream);

/* tld_sample_requests with one guidance value per FORWARD: guidance is a HOST array [batch, n_max], row b holding g[b][i] for
 * i = 0 .. requests[b].n_levels - 1 (the last entry belongs to the final prediction); entries past n_levels are ignored, every used entry must be
 * finite, and requests[b].class_guidance is ignored.  A forward whose g is not bit-equal to 1.0f is today's step: x0 = fma(g, cond, (1 - g) unc).
 * A forward whose g is 1.0f has NO unconditional model sample: x0 = cond, the value itself -- what the formula gives at g = 1 for finite unc, up to
 * the sign of a zero.  The model batch of step i is [B_i conditional samples | U_i unconditional samples], U_i = #{b < B_i : g[b][i] != 1} compacted in
 * request order, so the call makes sum(n_levels) + sum(U_i) model-sample forwards and needs max_i (B_i + U_i) <= max_batch (not 2 x batch).  Request
 * b's results do not depend on the other requests, on their tables, or on whether its own unguided steps were skipped or computed.  Limited-interval
 * guidance (guide only while sigma is inside [lo, hi]) is a table of g and 1.0 (schedule.guidance_table).  It records the launch-path bits 58-60 of
 * the tld_sample_requests step it runs.  The record checks come first and need no device; every refusal happens before anything is enqueued; no
 * stream synchronisation.  Test hook TLD_GUIDANCE_SKIP=0 (read at tld_engine_create): the full 2 B_i batch runs at every step and an unguided step
 * combines with the fma as if guided at g = 1; the capacity rule follows the batch actually run. */
TLD_API int tld_sample_requests_guided(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels,
               const void* neg_labels, const tld_sample_request* requests, const float* coeffs, const float* guidance, int32_t n_max, float sharp_f,
               float bright_f, void* out_latent, int32_t batch, void* trace_x0, void* trace_xt, void* hip_stream);
/* tld_sample_requests_guided with noise injected inside the step: SDE DPM-Solver++(2M) and DDIM with eta, per request.  Two more
 * HOST arrays:
 *   noise_coeff [batch, n_max] fp32: e of request b's forward i (schedule.step_coefficients(..., eta) returns it beside the table whose a, b, c it
 *               belongs to).  Every used entry must be finite and >= 0, and the entry of a request's final forward must be 0; entries past n_levels
 *               are ignored
 *   noise_keys  [batch] uint64: the request's noise key
 * After x_t = (a D + b x_t) / c of an inner step, and before the mask blend, the step adds x_t <- x_t + e z: the product is rounded, then the sum.
 * z are standard normals from Philox4x32-10 under the request's key at the counter (quad, i, tag, 0), quad = (element index inside the request's own
 * [C, S, S] image) / 4 and i the forward index of the request's own trajectory (csrc/tld_sampler_noise.h), through the Box-Muller functions of the
 * batch preparation.  Neither the request's place in the call nor the other requests enter the counter: request b's result is bit for bit that of
 * the request alone with the same key.  A forward whose e is 0.0f draws nothing and adds nothing, so an all-zero noise_coeff gives the result of
 * tld_sample_requests_guided -- or, with guidance NULL, of tld_sample_requests -- bit for bit.  With a mask the known region still rides the forward
 * process of the start eps; x0_prev, trace_x0 and trace_xt are written as before, trace_xt after the noise.
 *   guidance    as in tld_sample_requests_guided, or NULL: every forward of request b then takes requests[b].class_guidance and no unconditional
 *               sample is skipped -- the 2 B_i batch and the capacity rule (batch*2 <= max_batch) of tld_sample_requests
 * Still one elementwise launch per step; the second table (e and the key per (step, request)) travels in the same pinned staging upload as the rows,
 * no stream synchronisation.  tld_engine_sample_rows and the launch-path bits are those of the entry it generalises (58-60).  All record checks,
 * these arrays' included, come first and need no device; every refusal happens before anything is enqueued. */
TLD_API int tld_sample_requests_stochastic(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels,
               const void* neg_labels, const tld_sample_request* requests, const float* coeffs, const float* guidance, const float* noise_coeff,
               const uint64_t* noise_keys, int32_t n_max, float sharp_f, float bright_f, void* out_latent, int32_t batch, void* trace_x0,
               void* trace_xt, void* hip_stream);
/* engine-free: out_device [batch, img] fp32 <- the normals the stochastic step draws for request key keys_device[b] (uint64, device) at forward
 * steps_device[b] (uint32, device) over an image of img elements, from the device function the step kernel calls.  img need not be a multiple of 4 */
TLD_API int tld_debug_sampler_noise(const uint64_t* keys_device, const uint32_t* steps_device, int32_t batch, int32_t img, float* out_device,
               void* hip_stream);
/* tld_sample_requests_stochastic with a shape for the guidance update: guidance rescale and adaptive projected guidance, per request.
 * One more HOST array:
 *   shape [batch][4] fp32: (eta_par, norm_r, beta, phi) of request b.  eta_par: weight of the part of the update cond - unc parallel to cond (1: off);
 *         norm_r: the update's norm over the request's image is clipped to it (0: off); beta: momentum over the updates, d + beta m with m the
 *         previous guided forward's update, zero at the call's start (0: off; APG uses negative values); phi: guidance rescale, the standard deviation
 *         of the prediction over the request's image is pulled towards that of cond (0: off).  Refused: non-finite values, eta_par < 0, norm_r < 0,
 *         |beta| >= 1, phi outside [0, 1]
 * A request whose row is (1, 0, 0, 0) takes fma(g, cond, (1 - g) unc) as every other entry does, the same bits; so does every request at a forward
 * that runs no unconditional sample (x0 = cond) or is guided at exactly 1.0f, which neither reads nor writes the momentum.  Otherwise a launch of one workgroup per running
 * request sums cond, dbar, cond^2, dbar cond, dbar^2 over the request's whole image (a masked-out known region included) in double, in an order
 * that depends on the image size alone, makes two fp32 weights (csrc/tld_guidance_shape.h), and the step takes x0 = fma(P, cond, fl32(Q dbar)).
 * Request b's result is bit for bit that of the request alone.  A step in which no running request needs that launch does not make it.
 *   noise_coeff, noise_keys  as in tld_sample_requests_stochastic, or both NULL: no noise
 *   guidance                 as there, or NULL
 * tld_engine_sample_rows and the launch-path bits are those of the entry it generalises; the statistics launch is timed in the `update` class.
 * Every refusal happens before anything is enqueued; no stream synchronisation. */
TLD_API int tld_sample_requests_shaped(tld_engine* e, const void* noise, const void* init_latent, const void* mask, const void* labels,
               const void* neg_labels, const tld_sample_request* requests, const float* coeffs, const float* guidance, const float* noise_coeff,
               const uint64_t* noise_keys, const float* shape, int32_t n_max, float sharp_f, float bright_f, void* out_latent, int32_t batch,
               void* trace_x0, void* trace_xt, void* hip_stream);
/* engine-free: the statistics kernel and the combine of the shaped step on cond_device, unc_device [batch, img] fp32 under the HOST arrays g [batch]
 * and shape [batch][4]: x0_device [batch, img] fp32, pq_device [batch][2] fp32 (P, Q), sums_device [batch][5] double (sum c, sum dbar, sum c^2,
 * sum dbar c, sum dbar^2); zeros for a neutral row, whose x0 is plain CFG.  mom_device [batch, img] fp32 or NULL: read, and overwritten with dbar, for the
 * entries with beta != 0 (NULL: every beta must be 0).  img need not be a multiple of 4.  Returns after the stream has finished */
TLD_API int tld_debug_guidance_shape(const float* cond_device, const float* unc_device, float* mom_device, const float* g, const float* shape,
               int32_t batch, int32_t img, float* x0_device, float* pq_device, double* sums_device, void* hip_stream);
/* model samples the last sampler call on this engine enqueued: conditional and unconditional.  tld_sample / tld_sample_from / tld_sample_requests
 * report sum(n_levels) twice; tld_sample_requests_guided reports (sum(n_levels), sum(U_i)) */
TLD_API int tld_engine_sample_rows(tld_engine* e, int64_t* cond, int64_t* uncond);

/* SAMPLER SESSIONS: a sampler whose membership changes between steps.  A session holds `slots` slots of per-request state on one
 * engine; tld_session_admit puts a request into a free slot, tld_session_step runs ONE model forward for every live request, each at its own level,
 * and one elementwise update; a request leaves at its final forward.  A request's result is bit for bit that of tld_sample_requests (or _guided /
 * _stochastic) with that request alone: nothing of its arithmetic depends on its slot, its neighbours or the step it was admitted at.
 *   one session per engine; while it is open it owns the engine's conditioning tables and sampler buffers, and tld_denoiser_forward, the six
 *   tld_sample* entries and tld_engine_refresh_weights return TLD_ERR_STATE.  After tld_session_close they behave, and produce bits, as before.
 * A request: device noise [C, S, S], device label [text_emb], optional device negative label, n_levels with a HOST table [n_levels][6] as in
 * tld_sample_requests, a scalar class_guidance or a HOST table guidance [n_levels] (a forward guided at exactly 1.0f then runs no unconditional
 * sample, the engine's guidance-skip rule), and optionally HOST noise_coeff [n_levels] with a 64-bit key (HOST, one value) as in
 * tld_sample_requests_stochastic.  Every host array is copied by admit.  sharp_f / bright_f are per session.  Not part of a session, and without a
 * field here: init_latent, start_mix < 1, masks, the guidance shape (rescale / APG) and traces; `reserved` must be 0.
 * tld_session_open   TLD_ERR_STATE: weights not finalized, a session already open, a capturing stream.  TLD_ERR_INVALID: slots < 1,
 *                    2 slots > max_batch (every step then fits: no step is refused for its batch), cond_rows outside 3 .. 1024.  cond_rows is the
 *                    session's conditioning-row table: row 0 the zero label, per live request one label row (two with a negative label) and a shared,
 *                    reference-counted row per distinct float32 sigma.  The stream is the session's: admit and step take the stream again and are
 *                    refused on any other (TLD_ERR_INVALID), or while it is capturing (TLD_ERR_STATE).
 * tld_session_admit  *slot_out = the slot, or -1 with TLD_OK when there is no room NOW (no free slot, or too few free rows): ask again after a step.
 *                    TLD_ERR_INVALID: a bad record (the wording of tld_sample_requests where the rule is the same), or a request that could never
 *                    fit (its rows exceed cond_rows - 1).  Copies the noise into the slot, computes only the NEW conditioning rows in place.
 * tld_session_step   finished_slots [cap] <- the slots whose request ran its final forward in this step (ascending), *n_finished their number;
 *                    cap < slots is refused.  A step with no live request enqueues nothing.  Never synchronises the stream: the tables travel
 *                    through a ring of pinned staging buffers, each behind its own event.  With tld_engine_set_debug(1) the launch paths are
 *                    recorded (bit 62 for the session step) and no stage is kept.
 * tld_session_latent the [C, S, S] fp32 device result of a finished slot; it stays valid until a later admit reuses the slot, so a copy enqueued on
 *                    the session's stream before that admit reads the finished latent.
 * tld_session_stats  out[5] <- live requests, steps made, conditional and unconditional model samples so far, conditioning rows in use.
 * tld_session_close  frees the session (its three [slots, C, S, S] buffers stay with the engine's arena) and gives the engine back. */
typedef struct tld_session tld_session;
typedef struct tld_session_request {
    int32_t n_levels;             /* >= 2 */
    float class_guidance;         /* finite; read when guidance is NULL */
    int32_t has_negative;         /* != 0: the unconditional sample reads neg_label */
    int32_t reserved;             /* 0 */
    const float* coeffs;          /* HOST [n_levels][6] */
    const float* guidance;        /* HOST [n_levels] or NULL */
    const float* noise_coeff;     /* HOST [n_levels] or NULL */
    const uint64_t* noise_key;    /* HOST, one value; NULL exactly when noise_coeff is */
    const float* noise;           /* device [C, S, S] */
    const float* label;           /* device [text_emb] */
    const float* neg_label;       /* device [text_emb] or NULL */
} tld_session_request;
TLD_API int tld_session_open(tld_engine* e, int32_t slots, int32_t cond_rows, float sharp_f, float bright_f, void* hip_stream, tld_session** out);
TLD_API int tld_session_admit(tld_session* s, const tld_session_request* request, void* hip_stream, int32_t* slot_out);
TLD_API int tld_session_step(tld_session* s, void* hip_stream, int32_t* finished_slots, int32_t cap, int32_t* n_finished);
TLD_API int tld_session_latent(tld_session* s, int32_t slot, const float** device_ptr);
/* dst_device [C, S, S] fp32 <- the slot's result, a device copy enqueued on the session's stream (hip_stream: as in tld_session_step) */
TLD_API int tld_session_copy_latent(tld_session* s, int32_t slot, void* dst_device, void* hip_stream);
TLD_API int tld_session_stats(const tld_session* s, int64_t* out);
TLD_API int tld_session_close(tld_session* s);

/* THE STAGE HOOK: one contract behind tld_engine_ / tld_vae_ / tld_vae_enc_ / tld_clip_ / tld_train_ set_debug and read_stage (one implementation:
 * StageStore, csrc/tld_host.h).  set_debug(1) turns capture on, and twice is harmless; the engine's next calls keep named stages: the
 * engine's own buffers read in place, or device-to-device copies taken on the call's stream right after the kernel that completed the value, in
 * the stored type.  Every call forgets the copies of the call before it.  set_debug(0) and destroy free all of it.  read_stage converts a stage to
 * fp32 in its logical shape on the host and synchronises the device:
 *   TLD_ERR_KEY    the name is unknown or not captured (debug off, no debug call yet, a stage of another path);
 *   TLD_ERR_SHAPE  numel differs from the stage's element count: host_out is untouched; shape4, where the entry has one and it is not null,
 *                  holds the logical shape whenever the stage exists (unused trailing dimensions 1);
 *   TLD_ERR_STATE  from the CALL, when a copy finds no reserved memory (set_debug(1) before the engine's mode was chosen).
 * tld_debug_decode_stage is the store's decoder alone, for the CPU suite.  The blocks below list only what is each engine's own: its names, what it
 * poisons and when its snapshot memory is taken. */
#define TLD_STAGE_F32 0
#define TLD_STAGE_BF16 1
#define TLD_STAGE_U8 2        /* raw bytes */
#define TLD_STAGE_MX8S 3      /* E8M0 scale bytes stored [cols / 4][rows][4], logical [rows, cols] */
#define TLD_STAGE_MX8W 4      /* e4m3 codes [rows, cols] with scales `aux` [cols / 128][rows][4]: code x 2^(scale - 127) */
#define TLD_STAGE_PLAIN 0
#define TLD_STAGE_QKV_ROWS 1  /* 3 d rows in the fused QKV -> attention kernel's packed order -> [q; k; v] x [head][64] */
#define TLD_STAGE_NHWC 2      /* logical (B, C, H, W) stored [B][H][W][C] */
/* raw (host copy of the stored bytes; with outer_stride != 0: shape4[0] runs of shape4[1..3] elements, outer_stride elements apart) -> out fp32 [numel]
 * in logical order.  aux: TLD_STAGE_MX8W only; d, heads: TLD_STAGE_QKV_ROWS only.  No device is touched.  TLD_ERR_INVALID: a null pointer or an
 * impossible combination; TLD_ERR_SHAPE: numel is not the product of shape4. */
TLD_API int tld_debug_decode_stage(const void* raw, const void* aux, int32_t dtype, int32_t layout, const int64_t* shape4, int64_t outer_stride,
                                   int32_t d, int32_t heads, float* out, int64_t numel);

/* The inference forward's stages.  With debug on, a forward
 * (tld_denoiser_forward, or every step of tld_sample / tld_sample_from)
 *   - first fills every engine-owned activation, statistics, seam and split-K buffer -- and, once per call, the conditioning tables -- with 0xFF bytes
 *     (NaN in bf16 and fp32), so that a kernel that stores nothing, or too few rows, shows as NaN instead of the previous call's values;
 *   - keeps every stage of every block.  Snapshot memory (for max_batch samples) is allocated by set_debug(1), which fails cleanly
 *     (TLD_ERR_HIP, debug stays off) if it cannot be had, and freed by set_debug(0) / destroy; a forward allocates nothing.  Call set_debug(1) after
 *     tld_engine_set_low_latency;
 *   - records which launch path every size-dependent dispatch took (tld_engine_debug_paths).
 * With debug off nothing is launched, copied or allocated for the hook, and the outputs are bitwise the same.  A debug call on a capturing stream is
 * refused (TLD_ERR_STATE).  CFG layer-0 sharing stays on under debug: in a sampler step block 0's stages up to `att` hold the un-doubled batch.
 *
 * Stage names (i = block index; M = batch * tokens, Mi = the rows block i's first half runs on: src_batch * tokens for block 0 of a sampler step):
 *   tokens0 [Mi, d]; blk<i>.x_in [Mi, d] (the residual stream entering the block), blk<i>.ln1 [Mi, 8, 2] (the (sum, sum of squares) partial sums the
 *   LayerNorm-1 fold reads: the first 2 slots in block 0, d / 96 later; the others keep the poison) or blk<i>.xn1 [Mi, d] without the fold,
 *   blk<i>.qk [Mi, 2 d] and blk<i>.vt [samples, d, tokens] on the two-kernel path, blk<i>.att [Mi, d], blk<i>.sa [M, d] (x + att, fp32), blk<i>.ca
 *   [M, d], blk<i>.stats [M, 2] ((mean, rstd) of the stored row) or blk<i>.xn3 [M, d] without the LayerNorm-3 fold, blk<i>.hid_pre [M, hid] where
 *   the up-projection's output exists in HBM, blk<i>.hid [M, hid], blk<i>.splitk [splits, M, d] in the low-latency classes, blk<i>.mlp [M, d];
 *   the LAST block's blk<i>.mlp, where out_proj is folded into its down projection (default class, bf16 operands; TLD_FOLD_TAIL=0 turns the fold off): the
 *   product path never forms that row, so the stage is an fp32 evaluation x2 + hid Wd^T + bd made for the hook alone, in the hook's own memory
 *   (an fp32-output GEMM plus a row add; no product buffer is touched, no launch path recorded) -- `out` is the folded tail of blk<i>.ca and blk<i>.hid;
 *   out [batch, C S S] (the forward's output before any I/O cast); of a sampler's debug step: step.x_t, step.x0_prev (its inputs), step.out
 *   [2 B, C S S], step.x0, step.x_next (absent at the last step);
 *   conditioning, read in place: cond.sin [Tn, noise_embed_dims], cond.h1 [Tn, d] (the Tn noise rows: sinusoid features, GELU(ff1)), cond.pre, cond.y [T, d] (T token rows: noise rows, then label rows), cond.kv [L, T, 2 d], cond.wq [L, T, H, d],
 *   cond.bwq [L, T, H];
 *   operands as the engine holds them, read in place, in logical [N][K] order (the fused QKV -> attention kernel's row packing is undone on read):
 *   blk<i>.wqkv [3 d, d], blk<i>.wup [hid, d] (gamma-scaled under the LayerNorm folds), blk<i>.wdown [d, hid], and the folds' vectors
 *   blk<i>.qkv_c1, blk<i>.qkv_b1 [3 d], blk<i>.up_c1, blk<i>.up_b1 [hid].
 *   every other weight image, read in place in STORAGE order under img.<field> (an image the engine's mode does not hold: no such stage):
 *   the fp32 copies img.{angular [noise_embed_dims / 2], ff1_w [d, noise_embed_dims], ff1_b, ff3_w [d, d], ff3_b, label_w [d, text], label_b, norm_w, norm_b,
 *   conv_w [pd, pd], conv_b, pln1_w, pln1_b [pd], plin_b, pln2_w, pln2_b [d], pos [tokens, d], out_w [pd, d], out_b [pd]} (pd = patch_dim) and
 *   blk<i>.img.{kv_w [2 d, d], q_w [d, d], up_b, dw_b [hid], down_b, n1_w, n1_b, n2_w, n2_b, n3_w, n3_b [d]}; the split bf16 pairs img.out_w_hl
 *   [2, pd, d], img.plin_w_hl [2, d, pd], img.out_fold_hl [2, pd rounded up to 16, d + hid] with img.out_fold_b [pd]; img.plin_wt [pd, d];
 *   blk<i>.img.{qkv_wf [3 d, d], qkv_c1, qkv_b1 [3 d]} (the LayerNorm-1 fold in [q; k; v] row order) and blk<i>.img.{qkv_wp, qkv_c1p, qkv_b1p}, the same in
 *   the fused kernel's PACKED row order; blk<i>.img.{dw_w9c, dw_w9c_half [9, hid], dw_b_half [hid]} and blk<i>.img.dw_wpk [3, 4, hid, 2], the packed tap
 *   pairs as bf16 (low half first); fp8 mode: blk<i>.img.{qkv_w8 [3 d, d], up_w8 [hid, d], down_w8 [d, hid]}, the raw e4m3 codes, and
 *   blk<i>.img.{qkv_s8, up_s8, down_s8} [N, K / 32], the E8M0 scale bytes in logical order, both as the byte values 0 ... 255.
 *   fp8 GEMM mode (tld_engine_set_gemm_dtype; no folds, two-kernel QKV, up-projection alone): the three A operands as the GEMMs read them, copied after
 *   the producer or quantisation pass and before the GEMM: blk<i>.a8_qkv [Mi, d], blk<i>.a8_up [M, d], blk<i>.a8_down [M, hid], each as two stages:
 *   <name>.q, the e4m3 codes, and <name>.s [rows, K / 32], the E8M0 scale bytes in logical order (the GEMM's [K / 128][rows][4] layout, with the rows
 *   of the call, is undone on read); both read as the byte values 0 ... 255.  blk<i>.hid_pre is kept; blk<i>.xn1, blk<i>.xn3 and blk<i>.hid exist
 *   where a bf16 copy does (separate quantisation passes: TLD_FP8_FUSED=0, and the widths / grids whose producers do not quantise themselves) and
 *   are "no such stage" (TLD_ERR_KEY) elsewhere.  blk<i>.wqkv, blk<i>.wup, blk<i>.wdown return the e4m3 weights as held, DEQUANTISED on the host
 *   side of the read (code x 2^(scale - 127), exact in fp32).
 *   The first hook's names stay as aliases: cond_y, tokens0, blk0_sa, blk0_ca, blk0_mlp, tokens_final, blk0_hid, blk0_hid_pre.
 * Launch-path bits of tld_engine_debug_paths (bit number : path):
 *    0 embed plain   1-4 embed_mfma<2 | 4 | 6 | 8>   5-8 layernorm q4<1..4>   9 layernorm generic   10 layernorm mx8 (fp8 mode)
 *   11 QKV fused with attention   12 QKV with the LayerNorm-1 fold   13 QKV plain
 *   14 attention 256 tokens   15 chunked (k 256 tokens)   17 64 tokens   19 masked (any other count)   (18 unused: no square token grid has 32 tokens)
 *   16 out_proj folded into the last block's down projection (tail_fold_kernel; set together with the tail_mfma<NT> bit of its patch-feature tiles)
 *   20-23 cross_row_mfma<1..4>   24 ... with one 16-row group per workgroup   25 ... with more   26 cross_row VALU   27 the x_in fan-out (layer-0 sharing)
 *   28 up-projection fused with the depthwise conv, 16 x 16   29 ... 32 x 32 plus the seam kernel   30 ... 16 x 16, the 4-wave small-launch form
 *   31 up-projection alone   32 depthwise whole image   33 tiled   34 streaming
 *   35 down projection writing LayerNorm-1 partial sums   36 ... not writing them (last block, or no fold)   37 down projection, 8-wave kernel
 *   38 4-wave form, 64-row tiles   39 4-wave form, 128-row tiles   40 split-K x 4   41 split-K x 8   42 split-K 4-wave form
 *   43 split-K finisher <12> (d 768)   44 <6> (d 384)   45-48 tail_mfma<1..4>   49 tail plain (widths that are no multiple of 128, unfolded only)
 *   the sampler's step and start kernels, named by the entry that launched them: tld_sample 50 update; tld_sample_from 51 update_from without a mask
 *   52 update_from with a mask   53 start_mix
 *   writers of the MX-fp8 A operand (with bit 10): 54 separate quantisation pass   55 cross_row_mfma writing e4m3   56 depthwise tiled writing e4m3
 *   57 depthwise streaming writing e4m3
 *   tld_sample_requests: 58 update_requests without a mask   59 update_requests with a mask   60 start_mix per request
 *   61 fused QKV + attention on two-head tiles (set instead of bit 11 by such a launch)
 *   tld_session_step: 62 update_session (TLD_SESSION_PATH_BIT; the bits above are those of the closed sampler calls and the forward) */
#define TLD_ENGINE_PATH_BITS 61
#define TLD_SESSION_PATH_BIT 62
TLD_API int tld_engine_set_debug(tld_engine* e, int32_t enable);
TLD_API int tld_engine_read_stage(tld_engine* e, const char* name, float* host_out, int64_t numel);
/* logical shape of a captured stage: 4 int64, unused trailing dimensions 1 */
TLD_API int tld_engine_stage_shape(tld_engine* e, const char* name, int64_t* shape4);
/* sampler step (0-based) whose stages a debug tld_sample / tld_sample_from keeps; negative (the default): every step, so the last one remains */
TLD_API int tld_engine_set_debug_step(tld_engine* e, int32_t step);
/* mask of the launch paths the last debug call took */
TLD_API int tld_engine_debug_paths(tld_engine* e, uint64_t* mask);

/* Test hook: C[M,N] = A[M,K] . W[N,K]^T with the engine's bf16 MFMA GEMM (fp32 accumulate), bf16
 * device inputs, fp32 device output.  K % 64 == 0.  Refused (TLD_ERR_INVALID, nothing launched) when an operand row
 * starts beyond the reach of the GEMM's 32-bit DMA offsets: (M - 1) K 2 + 128 > 2^32, or the same for N. */
TLD_API int tld_debug_gemm_bf16(const void* a_bf16, const void* w_bf16, float* c_f32, int32_t M, int32_t N,
                        int32_t K, void* hip_stream);

/* Test hook: the same product as `ksplit` K-slices, c_slices[s] = A[:, s K/ksplit : (s+1) K/ksplit] . W[:, same]^T (fp32 [ksplit][M][N]).  K % (64 ksplit) == 0. */
TLD_API int tld_debug_gemm_splitk(const void* a_bf16, const void* w_bf16, float* c_slices_f32, int32_t M, int32_t N, int32_t K, int32_t ksplit,
                          void* hip_stream);

/* Test hooks of the MX-fp8 path.  quant_mx8: bf16 device matrix [M,K] -> e4m3 bytes [M,K] + E8M0 block scales laid out
 * [K/128][M][4] (device); quant_mx8_host: the weight-side quantiser (fp32 host matrix, host outputs, no GPU needed);
 * gemm_mx8: C[M,N] = dequant(A) . dequant(W)^T in fp32 from such operands (device).  K % 128 == 0, M % 4 == N % 4 == 0. */
TLD_API int tld_debug_quant_mx8(const void* in_bf16, void* out_e4m3, void* out_scale, int32_t M, int32_t K, void* hip_stream);
TLD_API int tld_debug_quant_mx8_host(const float* w, int32_t rows, int32_t K, void* out_e4m3, void* out_scale);
/* quant_mx8_f32: the weight-side quantiser on the device (fp32 device matrix [rows,K] -> device outputs laid out as above), the kernel
 * tld_engine_refresh_weights runs in the fp8 mode; its codes and scale bytes equal quant_mx8_host's on every input.  K % 128 == 0. */
TLD_API int tld_debug_quant_mx8_f32(const float* in_device, void* out_e4m3, void* out_scale, int32_t rows, int32_t K, void* hip_stream);
TLD_API int tld_debug_gemm_mx8(const void* a_e4m3, const void* a_scale, const void* w_e4m3, const void* w_scale, float* c_f32,
                               int32_t M, int32_t N, int32_t K, void* hip_stream);

/* Test/bench hook: time the engine's GEMM on self-allocated, pseudo-randomly filled device buffers.
 * epilogue: 0 fp32 out, 1 QKV (q|k row-major + V^T; N = 3*d, ntok tokens per sample), 2 bias+bf16,
 * 3 bias + fp32 residual add.  Returns the average kernel time over `iters` launches (HIP events). */
TLD_API int tld_debug_gemm_bench(int32_t M, int32_t N, int32_t K, int32_t epilogue, int32_t ntok, int32_t iters,
                                 double* avg_ms);

/* Test hook: ONE launch of the engine's GEMM with any of its non-conv epilogues on the caller's device buffers (tests/test_gpu_gemm_epilogues.py
 * holds every kernel class against float64).  The fields are GemmParams' (csrc/tld_gemm_params.h); unused ones stay 0 / NULL.
 *   epilogue 0: c_f32 [M][ldc] = A W^T.   2: out_bf16 [M][ldo] = bf16(A W^T + bias); with row_stats ([M] float2 (mean, rstd)) and ln_c1 [N] the folded
 *   LayerNorm-3, bf16(rstd_m (acc - mean_m c1[n]) + bias[n]).   3: resid [M][ldr] (bf16) += A W^T + bias, and with stats_out ([M][8] float2) the (sum, sum of
 *   squares) of the stored values per 96-column slot.   1: q | k -> out_bf16 [M][ldo >= 2 d], v -> vt [M / ntok][d][ntok].   5: epilogue 1 with LayerNorm-1
 *   folded in: ln_stats [M][8] float2 partial sums of the A rows, ln_slots of them summed, rstd_m (acc - mean_m ln_c1[n]) + ln_b1[n], mean over K.
 *   f8 != 0: A / W are e4m3 bytes with a_scale / w_scale as tld_debug_quant_mx8 lays them out (epilogues 0 - 3).
 *   w_batch_rows != 0 (epilogues 0 and 2, bf16): rows [g w_batch_rows, (g + 1) w_batch_rows) multiply the W matrix at byte offset g w_batch_stride_bytes.
 * Everything the kernels assume silently is checked first and refused with TLD_ERR_INVALID and the reason in tld_last_error(): operands the epilogue needs,
 * K % 64 (fp8: K % 128, M % 4, N % 4), 16-byte rows and pointers, N % 8 for the bf16-storing epilogues (N % 4 for the residual add), pitches, the QKV
 * geometry (N = 3 d, d % 64, ntok % 8, M % ntok), ln_slots even in 2 .. 8, an even M under row_stats, row_stats only without fp8 and where no 384-wide
 * tile can be chosen, stats_out only at the widths that have slots (N % 192 == 0, N <= 768, bf16).  Convolution mode, the fused depthwise epilogues
 * (4, 6) and fused attention (7) are refused: their layouts are engine-internal.
 * Sizes: the tile DMA reaches an operand row through a 32-bit byte offset -- (rows - 1) x pitch + 128 bytes <= 2^32 for A and for W (with the last group's
 * w_batch_stride_bytes offset), at most 2^24 rows, a pitch below 2^24 bytes -- refused with TLD_ERR_INVALID before the device is touched; the epilogues store
 * through 64-bit addresses, so outputs beyond 4 GiB are accepted. */
typedef struct tld_gemm_epilogue_args {
    const void* A; const void* W;                    /* bf16 [M][lda] / [N][ldw], K contiguous (fp8: bytes) */
    const void* a_scale; const void* w_scale;        /* fp8: E8M0 block scales [K / 128][rows][4] */
    const float* bias;                               /* [N] */
    void* out_bf16; void* vt; void* resid;
    void* stats_out; const void* ln_stats; const float* ln_c1; const float* ln_b1; const void* row_stats;
    float* c_f32;
    int32_t M, N, K, lda, ldw;
    int32_t epilogue, f8;
    int32_t ldo, ntok, d, ldr, ln_slots, ldc;
    int32_t w_batch_rows; uint32_t w_batch_stride_bytes;
} tld_gemm_epilogue_args;
TLD_API int tld_debug_gemm_epilogue(const tld_gemm_epilogue_args* args, void* hip_stream);

/* Test hook, host only (no GPU needed): which kernel, tile, K loop and grid a GEMM launch of the engine gets. `queries` holds n rows of
 * TLD_GEMM_PLAN_QUERY_INTS values --
 *   0 M, 1 N, 2 K, 3 lda, 4 ldw, 5 ldo, 6 ldr, 7 epilogue, 8 f8, 9 conv, 10 cv_cin, 11 cv_up, 12 cv_down, 13 ksplit, 14 w_batch_rows,
 *   15 / 16 / 17 whether bias / resid / c_f32 are present, 18 CU count of the device (> 0),
 *   19 - 23 the switches TLD_F8_RING, TLD_GEMM_HALFTAIL, TLD_UPDW_SMALL, TLD_SPLITK_SMALL, TLD_DOWN_SMALL (1 = on, their default)
 * -- and `plans` receives n rows of TLD_GEMM_PLAN_INTS values:
 *   0 family (0 refused: nothing would be launched, 1 the 8-wave kernel, 2 / 3 / 4 the 4-wave small-batch forms of the fused up-projection, the split-K
 *   slices and the residual-add down projection), 1 tile columns, 2 tile rows, 3 ring K loop, 4 xcd_ngroups, 5 half_tail, 6 workgroups, 7 threads per
 *   workgroup, 8 reason of a refusal (1 conv with cv_up and cv_down, 2 no kernel is built for the combination). */
#define TLD_GEMM_PLAN_QUERY_INTS 24
#define TLD_GEMM_PLAN_INTS 9
TLD_API int tld_debug_gemm_plan(const int32_t* queries, int32_t n, int32_t* plans);
/* Which form of the fused QKV + attention kernel a launch gets (tld_qkv_pair_plan.h: plan_qkv_pair): `queries` holds n rows of
 * (samples, heads, CU count), pair[i] receives 1 for two-head tiles and 0 for one-head tiles.  cost_ratio (may be null) receives numerator and
 * denominator of t_pair / t_item, the measured cost of a two-head tile in one-head items, which the rule compares whole rounds with. */
TLD_API int tld_debug_qkv_pair_plan(const int32_t* queries, int32_t n, int32_t* pair, int32_t* cost_ratio);

/* Live per-kernel-class timing with HIP events recorded on the launch stream around every launch
 * of the selected classes (bit k of class_mask).  Classes: 0 gemm_qkv, 1 gemm_up, 2 gemm_down,
 * 3 attention, 4 cross_row, 5 dwconv_gelu, 6 layernorm, 7 embed, 8 tail, 9 update, 10 conditioning.
 * set_profile forgets previously recorded timings; get_profile synchronises the device and returns
 * the summed elapsed time and the number of launches of one class since set_profile.
 * profile_reserve pre-creates `launches` event pairs for one class so that a timed region records into
 * existing events only (no hipEventCreate between the caller's fences). */
TLD_API int tld_engine_set_profile(tld_engine* e, uint32_t class_mask);
TLD_API int tld_engine_profile_reserve(tld_engine* e, int32_t kclass, int64_t launches);
TLD_API int tld_engine_get_profile(tld_engine* e, int32_t kclass, double* total_ms, int64_t* launches);

/* bytes of packed weights resident on the device */
TLD_API int64_t tld_engine_weight_bytes(const tld_engine* e);

TLD_API int tld_engine_destroy(tld_engine* e);

/* ---- VAE decode of the final latents --------------------------------------------------
 * Replaces `self.vae.decode(latents)[0]` at tld/diffusion.py:91, where `vae` is diffusers' AutoencoderKL
 * ("madebyollin/sdxl-vae-fp16-fix", tld/configs.py:39-43; a third-party dependency that is not part of the reference
 * checkout -- the algorithm restated here is AutoencoderKL.decode of diffusers 0.2x: post_quant_conv -> Decoder
 * (conv_in, UNetMidBlock2D with one single-head attention, UpDecoderBlock2D x n, GroupNorm + SiLU, conv_out)).
 * Activations are bf16 channels-last on the device, GroupNorm statistics / softmax / accumulation fp32. */
typedef struct tld_vae tld_vae;

typedef struct tld_vae_config {
    int32_t latent_channels;        /* 4 */
    int32_t out_channels;           /* 3 */
    int32_t n_blocks;               /* entries of block_out_channels in use (<= 4) */
    int32_t block_out_channels[4];  /* AutoencoderKL order, e.g. 128, 256, 512, 512; each in {64,128,256,512,1024} */
    int32_t layers_per_block;       /* 2: every decoder up block has layers_per_block + 1 resnets */
    int32_t norm_num_groups;        /* 32 */
    int32_t mid_block_attention;    /* 1 */
    int32_t use_post_quant_conv;    /* 1 */
    int32_t latent_size;            /* h = w of the latent image (32 for 256 px output) */
    int32_t max_batch;              /* largest batch one tld_vae_decode call will see */
    int32_t device_id;
} tld_vae_config;

TLD_API int tld_vae_create(const tld_vae_config* cfg, tld_vae** out);

/* AutoencoderKL.load_state_dict, one entry at a time (diffusers key names: "decoder.conv_in.weight",
 * "decoder.mid_block.attentions.0.to_q.weight" or its pre-0.19 spelling "...query.weight", "post_quant_conv.bias" ...).
 * "encoder.*" and "quant_conv.*" entries are accepted and ignored.  Host fp32 data. */
TLD_API int tld_vae_load_tensor(tld_vae* v, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim,
                                int32_t dtype);
TLD_API int tld_vae_finalize_weights(tld_vae* v);

/* AutoencoderKL.decode(z)[0] -- tld/diffusion.py:91.
 *   z    [batch, latent_channels, h, w]   device, io_dtype (already multiplied by the caller's scale factor)
 *   out  [batch, out_channels, 8h, 8w]    device, fp32 (2^(n_blocks-1) x upsampling) */
TLD_API int tld_vae_decode(tld_vae* v, const void* z, float* out, int32_t batch, int32_t io_dtype, void* hip_stream);

/* The decoder's stages (the stage hook above): bf16 NHWC copies of the activation after every stage, read as fp32 [batch, C, H, W]; their memory is
 * taken at capture, since the sizes follow the call's resolution.  names: "conv_in", "mid.res0", "mid.attn", "mid.res1", "up<i>.res<j>", "up<i>.upsample",
 * "norm_out".  shape4 (optional) receives batch, C, H, W. */
TLD_API int tld_vae_set_debug(tld_vae* v, int32_t enable);
TLD_API int tld_vae_read_stage(tld_vae* v, const char* name, float* host_out, int64_t numel, int64_t* shape4);

/* Live timing of one kernel class of the decoder (HIP events around every launch, like tld_engine_set_profile).
 * classes: 0 conv3x3, 1 gemm (1x1 / attention), 2 groupnorm, 3 other */
TLD_API int tld_vae_set_profile(tld_vae* v, int32_t enable);
TLD_API int tld_vae_get_profile(tld_vae* v, int32_t kclass, double* total_ms, int64_t* launches);

/* Test hook: the implicit-GEMM 3x3 convolution alone (zero padding 1, stride 1; up = 1: nearest 2x upsampling folded in).
 *   in  bf16 channels-last [B, H >> up, W >> up, cin] (device);  w  bf16 [cout][3][3][cin] (device)
 *   out fp32 [B*H*W][cout] (device).  cin % 64 == 0.  Synchronises the stream. */
TLD_API int tld_debug_conv3x3(const void* in_bf16, const void* w_bf16, float* out_f32, int32_t B, int32_t H, int32_t W,
                              int32_t cin, int32_t cout, int32_t up, void* hip_stream);

TLD_API int64_t tld_vae_weight_bytes(const tld_vae* v);
TLD_API int tld_vae_destroy(tld_vae* v);

/* ---- VAE encode: images -> latent moments (the reference's data pipeline, tld/data.py) --------------------------------
 * Replaces `vae.encode(x, return_dict=False)[0]` of tld/data.py, with the same third-party AutoencoderKL as the decoder above.
 * Restated: AutoencoderKL.encode of diffusers 0.2x -- Encoder (conv_in, DownEncoderBlock2D x n with Downsample2D(padding=0),
 * UNetMidBlock2D with one single-head attention, GroupNorm + SiLU, conv_out -> 2 latent_channels) and quant_conv 1x1.  The
 * DiagonalGaussianDistribution over the moments (mean | logvar) is evaluated by the caller.  Same numerics as the decoder. */
typedef struct tld_vae_enc tld_vae_enc;

typedef struct tld_vae_enc_config {
    int32_t in_channels;            /* 3 (1..4) */
    int32_t latent_channels;        /* 4 (<= 16): the moments have 2 latent_channels channels */
    int32_t n_blocks;               /* entries of block_out_channels in use (<= 4) */
    int32_t block_out_channels[4];  /* AutoencoderKL order, e.g. 128, 256, 512, 512; each in {64,128,256,512,1024} */
    int32_t layers_per_block;       /* 2: every encoder down block has layers_per_block resnets */
    int32_t norm_num_groups;        /* 32 */
    int32_t mid_block_attention;    /* 1 */
    int32_t use_quant_conv;         /* 1 */
    int32_t image_size;             /* S = h = w of the input image: a multiple of 64 and of 8 * 2^(n_blocks-1), 64..2048 */
    int32_t max_batch;              /* largest batch one tld_vae_enc_encode call will see (activation buffers < 4 GiB) */
    int32_t device_id;
} tld_vae_enc_config;

TLD_API int tld_vae_enc_create(const tld_vae_enc_config* cfg, tld_vae_enc** out);
/* AutoencoderKL.load_state_dict, one entry at a time (diffusers key names: "encoder.conv_in.weight",
 * "encoder.down_blocks.<i>.resnets.<j>.*", "encoder.down_blocks.<i>.downsamplers.0.conv.*", "encoder.mid_block.*" with the
 * pre-0.19 attention spellings accepted, "encoder.conv_norm_out.*", "encoder.conv_out.*", "quant_conv.*").  "decoder.*" and
 * "post_quant_conv.*" entries are accepted and ignored.  Host fp32 data. */
TLD_API int tld_vae_enc_load_tensor(tld_vae_enc* e, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim,
                                    int32_t dtype);
TLD_API int tld_vae_enc_finalize_weights(tld_vae_enc* e);
/* AutoencoderKL.encode(x).latent_dist.parameters -- tld/data.py.
 *   x        [batch, in_channels, S, S]                 device, io_dtype (already mapped to [-1, 1] by the caller)
 *   moments  [batch, 2 latent_channels, S/2^(n-1), S/2^(n-1)]  device, fp32 (mean, then logvar before its clamp) */
TLD_API int tld_vae_enc_encode(tld_vae_enc* e, const void* x, float* moments, int32_t batch, int32_t io_dtype, void* hip_stream);
/* The encoder's stages, as the decoder's.  names: "conv_in", "down<i>.res<j>", "down<i>.downsample", "mid.res0", "mid.attn",
 * "mid.res1", "norm_out" (after SiLU). */
TLD_API int tld_vae_enc_set_debug(tld_vae_enc* e, int32_t enable);
TLD_API int tld_vae_enc_read_stage(tld_vae_enc* e, const char* name, float* host_out, int64_t numel, int64_t* shape4);
/* Live timing per kernel class, as tld_vae_set_profile: 0 conv3x3, 1 gemm (1x1 / attention), 2 groupnorm, 3 other (conv_in, tail) */
TLD_API int tld_vae_enc_set_profile(tld_vae_enc* e, int32_t enable);
TLD_API int tld_vae_enc_get_profile(tld_vae_enc* e, int32_t kclass, double* total_ms, int64_t* launches);
TLD_API int64_t tld_vae_enc_weight_bytes(const tld_vae_enc* e);
TLD_API int tld_vae_enc_destroy(tld_vae_enc* e);

/* Test hook: the implicit-GEMM 3x3 convolution with stride 2 and padding (0, 1, 0, 1) (Downsample2D) alone.  H x W is the OUTPUT size.
 *   in  bf16 channels-last [B, 2H, 2W, cin] (device);  w  bf16 [cout][3][3][cin] (device)
 *   out fp32 [B*H*W][cout] (device).  cin % 64 == 0.  Synchronises the stream. */
TLD_API int tld_debug_conv3x3_s2(const void* in_bf16, const void* w_bf16, float* out_f32, int32_t B, int32_t H, int32_t W,
                                 int32_t cin, int32_t cout, void* hip_stream);

/* ---- CLIP text tower: the front edge ---------------------------------------------------
 * Replaces `model.encode_text(text_tokens)` in encode_text, tld/diffusion.py:136-140, where `model` is OpenAI CLIP
 * "ViT-L/14" from `clip.load` (tld/diffusion.py:160, tld/configs.py:46-48; third-party, not in the reference checkout).
 * Restated: CLIP.encode_text of openai/CLIP clip/model.py (token + positional embedding, pre-LN residual blocks with
 * causal nn.MultiheadAttention and a QuickGELU MLP, ln_final, the EOT token's row times text_projection).  Tokenisation
 * stays on the host (clip.tokenize); the engine takes token ids. */
typedef struct tld_clip tld_clip;

typedef struct tld_clip_config {
    int32_t vocab_size;         /* 49408 */
    int32_t context_length;     /* 77 (<= 128) */
    int32_t width;              /* 768: transformer width, multiple of 64 */
    int32_t heads;              /* width / 64 */
    int32_t layers;             /* 12 */
    int32_t embed_dim;          /* 768: columns of text_projection */
    int32_t max_batch;
    int32_t device_id;
} tld_clip_config;

TLD_API int tld_clip_create(const tld_clip_config* cfg, tld_clip** out);
/* CLIP.state_dict() entries, one at a time (host fp32): "token_embedding.weight", "positional_embedding", "text_projection",
 * "ln_final.*", "transformer.resblocks.<i>.{ln_1,ln_2}.*", ".attn.in_proj_{weight,bias}", ".attn.out_proj.*", ".mlp.c_fc.*",
 * ".mlp.c_proj.*".  "visual.*", "logit_scale" and the archive's metadata entries are accepted and ignored. */
TLD_API int tld_clip_load_tensor(tld_clip* c, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype);
TLD_API int tld_clip_finalize_weights(tld_clip* c);
/* CLIP.encode_text(text):  tokens [batch, context_length] int32 (device), eot_index [batch] int32 (device) = text.argmax(-1)
 * (the EOT token has the largest id), out [batch, embed_dim] fp32 (device). */
TLD_API int tld_clip_encode_text(tld_clip* c, const int32_t* tokens, const int32_t* eot_index, float* out, int32_t batch, void* hip_stream);
/* The text tower's stages (the stage hook above).  With debug on, tld_clip_encode_text
 *   - first fills every workspace buffer (x, tmp, pooled, h, qkv, att, f; all max_batch prompts) with 0xFF bytes -- NaN in bf16 and fp32 -- so that a kernel
 *     that stores nothing, or too few rows, shows as NaN instead of the previous call's values;
 *   - keeps every stage of every block.  Snapshot memory (for max_batch prompts: about 44 width bytes per row per block) is allocated by set_debug(1), which fails
 *     cleanly (TLD_ERR_HIP, debug stays off) if it cannot be had, and freed by set_debug(0) / destroy; an encode allocates nothing.
 * With debug off nothing is launched, copied or allocated for the hook, and the output is bitwise the same.  A debug call on a capturing stream is refused
 * (TLD_ERR_STATE).  Stages hold the LAST encode_text call (T = batch * context_length rows, W = width, E = embed_dim, i = block index):
 *   x0 [T, W] fp32 (token + positional embedding);
 *   blk<i>.h1 [T, W] bf16 (ln_1), blk<i>.qkv [T, 3 W] bf16, blk<i>.att [T, W] bf16, blk<i>.attn_out [T, W] fp32 (out_proj without its bias),
 *   blk<i>.x1 [T, W] fp32 (the stream after the first residual add), blk<i>.h2 [T, W] bf16 (ln_2), blk<i>.f_pre [T, 4 W] bf16 (c_fc + bias, before the
 *   in-place QuickGELU), blk<i>.f [T, 4 W] bf16, blk<i>.mlp_out [T, W] fp32 (c_proj without its bias), blk<i>.x2 [T, W] fp32 (the stream after the second
 *   add; absent for the last block, where only the pooled rows are formed);
 *   pooled [batch, W] fp32 (ln_final of the EOT rows), out [batch, E] fp32;
 *   operands as the engine holds them, read in place, logical [N][K]: blk<i>.in_w [3 W, W], blk<i>.out_w [W, W], blk<i>.fc_w [4 W, W], blk<i>.proj_w
 *   [W, 4 W] (bf16) and proj_t [E, W] (fp32, text_projection transposed); these are named from finalize_weights on and need no debug call.
 * shape4 receives (rows, columns, 1, 1). */
TLD_API int tld_clip_set_debug(tld_clip* c, int32_t enable);
TLD_API int tld_clip_read_stage(tld_clip* c, const char* name, float* host_out, int64_t numel, int64_t* shape4);
TLD_API int64_t tld_clip_weight_bytes(const tld_clip* c);
TLD_API int tld_clip_destroy(tld_clip* c);

/* ---- CLIP image tower: image embeddings in the labels' joint space ------------------------------------------------
 * Restated: VisionTransformer.forward of openai/CLIP clip/model.py, what `model.encode_image(preprocess(img))` runs: conv1 (patch x patch,
 * stride patch, no bias), class token + positional embedding, ln_pre, pre-LN residual blocks with unmasked nn.MultiheadAttention and a
 * QuickGELU MLP, ln_post of the class token's row times proj.  Resizing, cropping and normalising the picture stay in Python (clip_preprocess).
 * Limits, checked by tld_clip_vis_create before any HIP call (TLD_ERR_INVALID, the reason in tld_last_error()):
 *   width a multiple of 64 in 64..1024;  heads * 64 == width;  layers 1..64;  patch_size 1..32;  image_size a positive multiple of patch_size;
 *   g = image_size / patch_size in 1..16, i.e. at most 257 tokens (the 336 px towers, 577 tokens, are out of scope);  embed_dim, max_batch >= 1. */
typedef struct tld_clip_vis tld_clip_vis;

typedef struct tld_clip_vis_config {
    int32_t image_size;         /* 224: input_resolution */
    int32_t patch_size;         /* 14 */
    int32_t width;              /* 1024: vision_width, multiple of 64 */
    int32_t heads;              /* width / 64 */
    int32_t layers;             /* 24 */
    int32_t embed_dim;          /* 768: columns of visual.proj */
    int32_t max_batch;
    int32_t device_id;
} tld_clip_vis_config;

TLD_API int tld_clip_vis_create(const tld_clip_vis_config* cfg, tld_clip_vis** out);
/* CLIP.state_dict() entries, one at a time (host fp32): "visual.class_embedding" [W], "visual.positional_embedding" [g*g + 1, W], "visual.proj" [W, E],
 * "visual.conv1.weight" [W, 3, p, p], "visual.ln_pre.*", "visual.ln_post.*", "visual.transformer.resblocks.<i>.{ln_1,ln_2}.*",
 * ".attn.in_proj_{weight,bias}", ".attn.out_proj.*", ".mlp.c_fc.*", ".mlp.c_proj.*".  The text side of the archive, "logit_scale" and the
 * metadata entries are accepted and ignored. */
TLD_API int tld_clip_vis_load_tensor(tld_clip_vis* c, const char* key, const void* host_ptr, const int64_t* shape, int32_t ndim, int32_t dtype);
TLD_API int tld_clip_vis_finalize_weights(tld_clip_vis* c);
/* VisionTransformer.forward(pixels):  pixels [batch, 3, image_size, image_size] (device; io_dtype TLD_DTYPE_F32 / BF16 / F16), already normalised;
 * out [batch, embed_dim] fp32 (device).  Launches only: allocates nothing, does not synchronise. */
TLD_API int tld_clip_vis_encode_image(tld_clip_vis* c, const void* pixels, float* out, int32_t batch, int32_t io_dtype, void* hip_stream);
/* The image tower's stages (the stage hook above): the contract of tld_clip_set_debug -- every workspace buffer of all max_batch images
 * is filled with 0xFF bytes first, a capturing stream is refused (TLD_ERR_STATE), nothing is launched or allocated with the hook off and the output keeps
 * its bits.  Stages of the LAST encode_image call (P = batch * g*g patch rows, T = batch * (g*g + 1) token rows, Kp = 3 p*p rounded up to a multiple of 64):
 *   patches [P, Kp] bf16 (im2col rows, zero beyond 3 p*p), emb [P, W] fp32 (conv1), x0 [T, W] fp32 (after ln_pre);
 *   blk<i>.{h1, qkv, att, attn_out, x1, h2, f_pre, f, mlp_out, x2} as in the text tower (x2 absent for the last block);
 *   pooled [batch, W] fp32 (ln_post of the class rows), out [batch, E] fp32;
 *   operands as held, from finalize_weights on: conv_w [W, Kp] bf16, blk<i>.in_w / out_w / fc_w / proj_w (bf16), proj_t [E, W] fp32. */
TLD_API int tld_clip_vis_set_debug(tld_clip_vis* c, int32_t enable);
TLD_API int tld_clip_vis_read_stage(tld_clip_vis* c, const char* name, float* host_out, int64_t numel, int64_t* shape4);
/* The image tower's attention kernel alone (no engine): qkv_bf16 [batch * n, 3 * 64 heads] bf16 device rows as the in_proj GEMM leaves them (q | k | v,
 * head h at columns h * 64), out_bf16 [batch * n, 64 heads] bf16; unmasked softmax(q k^T / 8) v per (sample, head).  Reads rows 0 .. batch n - 1 of qkv and
 * stores rows 0 .. batch n - 1 of out, nothing else.  TLD_ERR_INVALID before any HIP call: a NULL pointer, batch < 1, n outside 2..257, heads outside 1..16. */
TLD_API int tld_debug_clip_vis_attention(const void* qkv_bf16, void* out_bf16, int32_t batch, int32_t n, int32_t heads, void* hip_stream);
TLD_API int64_t tld_clip_vis_weight_bytes(const tld_clip_vis* c);
TLD_API int tld_clip_vis_destroy(tld_clip_vis* c);

TLD_API const char* tld_last_error(void);

/* ---- Training step: tld/train.py:162-173 for one batch on one device -------------------------------------------
 * The model's parameters, their gradients, Adam's two moment vectors and the EMA copy are FLAT fp32 device vectors owned by the
 * caller, in the order of Denoiser.named_parameters() (tld/denoiser.py:85-114); tld_train_param_layout enumerates (key, offset,
 * numel).  The gradient all-reduce of the reference's accelerate/DDP wrapper (tld/train.py:114,168) is the caller's
 * torch.distributed all_reduce on the flat gradient vector between tld_train_forward_backward and tld_train_adam_ema.
 * cfg.max_batch = largest batch (NOT doubled); square latent grids of G x G tokens, G = image_size / patch_size a multiple of 4 with
 * 4 <= G <= 64 (16 .. 4096 tokens: the inference engine's grids up to 64 x 64; e.g. 576 tokens = 384 px at patch 2). */
typedef struct tld_train tld_train;
TLD_API int tld_train_create(const tld_config* cfg, tld_train** out);
TLD_API int64_t tld_train_param_count(const tld_train* e);
TLD_API int32_t tld_train_tensor_count(const tld_train* e);
TLD_API int tld_train_param_layout(const tld_train* e, int32_t index, char* key_out, int32_t key_cap, int64_t* offset, int64_t* numel);
/* registered buffer "fourier_feats.0.angular_speeds" (tld/transformer_blocks.py:11-15): host fp32 [noise_embed_dims / 2] */
TLD_API int tld_train_set_angular_speeds(tld_train* e, const float* host, int32_t n);
/* params / grads: device fp32 [tld_train_param_count] */
TLD_API int tld_train_bind(tld_train* e, float* params, float* grads);
/* bf16 GEMM operands (and their transposes) of the current parameters; called automatically after an optimizer step */
TLD_API int tld_train_refresh_weights(tld_train* e, void* hip_stream);
/* model.train(); pred = model(x_noisy, noise_level.view(-1, 1), label); loss = nn.MSELoss()(pred, target); loss.backward()
 * -- tld/train.py:160,166-168.  x_noisy / target [batch, C, S, S], noise_level [batch], label [batch, text_emb]: device fp32.
 * Writes every gradient into the bound grads vector (overwritten, like zero_grad + backward), the scalar loss to loss_out (device
 * fp32[1]) and the prediction to pred_out (device fp32 [batch, C, S, S]). */
TLD_API int tld_train_forward_backward(tld_train* e, const float* x_noisy, const float* noise_level, const float* label, const float* target,
                                       int32_t batch, float* loss_out, float* pred_out, void* hip_stream);
/* The same step with a host callback for overlapping the data-parallel gradient reduction with the backward pass -- what the bucketed
 * all-reduce hooks of the reference's DDP wrapper do (accelerate.prepare -> torch DDP, tld/train.py:109,168).  grad_ready(user, offset,
 * numel) is invoked on the calling thread each time the kernels that FINISH a contiguous range [offset, offset + numel) of the flat
 * gradient vector have been enqueued on hip_stream: once per decoder block, last block first (a block's 15 tensors are contiguous in
 * named_parameters() order), then the ranges before and after the blocks (embedding / position table; out_proj, norm, label_proj --
 * final only at the end of the backward).  The ranges tile the vector exactly.  The callback typically records an event on hip_stream
 * and launches an asynchronous all-reduce of that slice on a second stream; it must not synchronise hip_stream.  NULL: no callbacks. */
typedef void (*tld_grad_ready_fn)(void* user, int64_t offset, int64_t numel);
TLD_API int tld_train_forward_backward_cb(tld_train* e, const float* x_noisy, const float* noise_level, const float* label, const float* target,
                                          int32_t batch, float* loss_out, float* pred_out, void* hip_stream, tld_grad_ready_fn grad_ready, void* user);
/* optimizer.step() of torch.optim.Adam(lr) + update_ema(ema_model, model, alpha) -- tld/train.py:87,169,55-58,172.  step counts from 1;
 * ema may be NULL; grad_scale multiplies the gradient first (1 / world_size after a SUM all-reduce). */
TLD_API int tld_train_adam_ema(tld_train* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel,
                               float lr, float beta1, float beta2, float eps, int32_t step, float ema_alpha, float grad_scale, void* hip_stream);
/* The guarded optimizer step: clip_grad_norm_ (tld has none; torch.nn.utils.clip_grad_norm_ semantics) and the non-finite step skip of
 * accelerate's GradScaler (Accelerator(mixed_precision="fp16"), tld/train.py:69), decided ON THE DEVICE: neither call makes the host wait.
 * opt_state: caller-owned device fp64 [TLD_TRAIN_OPT_STATE_DOUBLES], all zeros = a fresh optimizer:
 *   [0] t: optimizer steps applied     [1] steps skipped in total     [2] last_skipped (0 or 1)
 *   [3] gradient norm of this step (of grads * grad_scale, before clipping; Inf or NaN when an element is non-finite)
 *   [4] clip coefficient     [5] bc1 = 1 - beta1^t     [6] bc2 = 1 - beta2^t     [7] 0     [8 ..] 1024 partial sums of squares
 * tld_train_grad_guard sums (grads[i] * grad_scale)^2 in double (fixed order, no atomics: bitwise repeatable; non-finite exactly when an
 * element is) and applies, in double:
 *   norm = sqrt(sum);  nonfinite = !isfinite(sum)
 *   if (skip_nonfinite && nonfinite)  skipped += 1; last_skipped = 1; coef = 0;  t, bc1, bc2 unchanged
 *   else  last_skipped = 0; t += 1; c = max_norm / (norm + 1e-6); coef = clip ? (c > 1 ? 1 : c) : 1;  bc1, bc2 from the new t
 * (clip = max_norm > 0 and finite; the bias corrections use the float-rounded betas; a NaN norm with the skip off gives a NaN coefficient,
 * as clip_grad_norm_(error_if_nonfinite=False) does).  TLD_ERR_INVALID before any HIP call: grads or opt_state NULL, numel <= 0, max_norm
 * NaN, grads not 16-byte or opt_state not 8-byte aligned.  e may be NULL.
 * tld_train_adam_ema_guarded is tld_train_adam_ema on gi = (grads[i] * grad_scale) * (float)coef with bc1 / bc2 read from opt_state; when
 * last_skipped is set it touches nothing.  e and ema may be NULL. */
#define TLD_TRAIN_OPT_STATE_DOUBLES (8 + 1024)
TLD_API int tld_train_grad_guard(tld_train* e, const float* grads, int64_t numel, float grad_scale, double max_norm, int32_t skip_nonfinite,
                                 float beta1, float beta2, double* opt_state, void* hip_stream);
TLD_API int tld_train_adam_ema_guarded(tld_train* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel,
                                       float lr, float beta1, float beta2, float eps, float ema_alpha, float grad_scale, const double* opt_state,
                                       void* hip_stream);
/* The grouped optimizer step: torch.optim.AdamW (decoupled weight decay) with parameter groups, a learning-rate schedule that follows the steps
 * APPLIED (LambdaLR behind accelerate's scheduler wrapper: no advance on a skipped step) and frozen tensors, behind the same guard.  A plan
 * describes the flat vector once: segment s (a tensor) has seg_numel[s] >= 1 elements -- the segments tile [0, numel) in order, any length, also not
 * a multiple of 4 -- and belongs to groups[seg_group[s]] = (lr_scale, weight_decay, frozen).  tld_opt_plan_create cuts every segment from its first
 * element into chunks of at most 8192 elements (a constant: not a function of the CU count; no chunk spans two segments), uploads the tables once
 * and owns the partial sums; a step allocates nothing and synchronises nothing.  lr_factors[n_factors] (may be NULL with n_factors = 0: factor 1):
 * applied step t = 1, 2, ... runs at factor lr_factors[min(t, n_factors) - 1].
 * opt_state is tld_train_grad_guard's vector with the same head; [7] holds the schedule factor, [8 ..] is not used by these calls.
 * tld_train_grad_guard_grouped, in double, fixed order, no atomics (bitwise repeatable on any CU count):
 *   partial[c] = sum over chunk c of (grads[i] * grad_scale)^2       (per thread as tld_train_grad_guard, then the fixed 256-lane tree)
 *   seg[s]     = partial[c] added in chunk order over the chunks of segment s       -> tld_opt_plan_segment_sqsums (frozen segments included)
 *   sum        = seg[s] added in segment order over the segments whose group is NOT frozen;  norm = sqrt(sum);  nonfinite = !isfinite(sum)
 *   if (skip_nonfinite && nonfinite)  skipped += 1; last_skipped = 1; coef = 0;  t, bc1, bc2 and [7] unchanged
 *   else  last_skipped = 0; t += 1; c = max_norm / (norm + 1e-6); coef = clip ? (c > 1 ? 1 : c) : 1;  bc1, bc2 from the new t;
 *         [7] = (double)lr_factors[min(t, n_factors) - 1] with the new t, or 1.0 without a table
 * tld_train_adamw_ema_grouped: a skipped step touches nothing; an element of a frozen group is neither read nor written (params, moments, EMA);
 * every other element i of group q, with bc1 / bc2 / coef read from opt_state:
 *   lr_q = (float)((double)lr * (double)lr_scale_q * [7]);   gi = (grads[i] * grad_scale) * (float)coef;   m, v as tld_train_adam_ema_guarded
 *   p = p * (1.0f - lr_q * wd_q)                  (AdamW: param.mul_(1 - lr * weight_decay); a product of its own, exact when wd_q = 0)
 *   p = p - (lr_q / bc1) * (m / (sqrtf(v) / sqrtf(bc2) + eps));   ema = ema * alpha + p * (1 - alpha)   (ema may be NULL)
 * so one group (1, 0, not frozen) without a table gives tld_train_adam_ema_guarded's bits.  A plan whose groups are all frozen is legal: norm 0,
 * the step counts and nothing else changes.
 * TLD_ERR_INVALID with a text naming the offending index, before any HIP call in tld_opt_plan_create: a null pointer, n_seg < 1, a segment length
 * < 1, n_groups outside 1 .. 256, a seg_group out of range, an lr_scale / weight_decay / factor that is negative or not finite, frozen not 0 / 1,
 * n_factors < 0 or > 0 with a null table, a total length over 2^40, more than 2^30 chunks; in the two step calls: a null pointer, numel !=
 * tld_opt_plan_numel, NaN max_norm, vectors not 16-byte or opt_state not 8-byte aligned.  A refusal enqueues nothing. */
typedef struct tld_opt_group { float lr_scale; float weight_decay; int32_t frozen; int32_t reserved; } tld_opt_group;
typedef struct tld_opt_plan tld_opt_plan;
TLD_API int tld_opt_plan_create(int32_t device, const int64_t* seg_numel, const int32_t* seg_group, int32_t n_seg, const tld_opt_group* groups,
                                int32_t n_groups, const float* lr_factors, int64_t n_factors, tld_opt_plan** out);
TLD_API void tld_opt_plan_destroy(tld_opt_plan* p);
TLD_API int64_t tld_opt_plan_numel(const tld_opt_plan* p);
TLD_API int tld_opt_plan_segment_sqsums(const tld_opt_plan* p, const double** device_ptr);        /* device double [n_seg], of the last guard call */
TLD_API int tld_train_grad_guard_grouped(tld_opt_plan* p, const float* grads, int64_t numel, float grad_scale, double max_norm, int32_t skip_nonfinite,
                                         float beta1, float beta2, double* opt_state, void* hip_stream);
TLD_API int tld_train_adamw_ema_grouped(tld_opt_plan* p, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t numel,
                                        float lr, float beta1, float beta2, float eps, float ema_alpha, float grad_scale, const double* opt_state,
                                        void* hip_stream);
/* The training batch of one step, built on the device from a resident dataset (tld/train.py:121-138 without the host):
 * gather rows idx[b] of the source, draw noise, noise level and label mask from Philox4x32-10 and mix.  One kernel on hip_stream; nothing is
 * allocated, nothing synchronises.  e may be NULL (the device is that of x_noisy).
 *   src        latents [rows, latent_elems] (latent_elems = C S S) as TLD_DTYPE_U8 / F16 / F32, labels [rows, text_emb] as F16 / F32, both device;
 *              TLD_DTYPE_U8: target = dequant_table[code] (device float[256], already divided by the VAE scale factor);
 *              F16 / F32: target = float(latent) / vae_scale, a correctly rounded fp32 division (tld/train.py:122)
 *   idx        device int64 [batch]; an index outside [0, rows) is never dereferenced: the position takes row 0 and *bad_index_count
 *              (device int32, never reset here) is incremented
 *   seed, step, replica   Philox key (seed_lo, seed_hi), counter (c0, 4 replica + stream, step_lo, step_hi); every draw is a function of
 *              (seed, replica, step, position) alone
 *     stream 0 noise: c0 = e / 4 of the flat element e of [batch, latent_elems]; words (r0, r1) and (r2, r3) give two Box-Muller pairs
 *              sqrt(-2 ln u0) (cos, sin)(2 pi u1), u = ((r >> 8) + 0.5) 2^-24 (ln u0 from log1p of the exact 1 - u0 where fp32 cannot hold u0)
 *     stream 1 noise level: one Beta(beta_a, beta_b) draw per sample in double, c0 = 64 b + j (the method and its loop bound: DESIGN.md 7.11)
 *     stream 2 label mask: c0 = b / 4, word b % 4, u = float(r >> 8) 2^-24; the label row is all zeros when u < label_dropout
 *   x_noisy = float(nl noise + (1 - nl) target) with every product and sum rounded in double, no FMA (= train.mix_noise bit for bit);
 *   noise_level = float(nl); label [batch, text_emb]; target [batch, latent_elems]: device fp32.
 *   noise (fp32 [batch, latent_elems]), noise_level64 (fp64 [batch]), mask (uint8 [batch]): what was drawn, for tests; each may be NULL.
 * TLD_ERR_INVALID before any HIP call: a NULL src, source pointer, idx, required output or bad_index_count; batch, rows, latent_elems or
 * text_emb <= 0; batch > 2^26 or batch * latent_elems > 2^34 (the 32-bit c0); an unknown dtype; TLD_DTYPE_U8 without a table; a float source
 * whose vae_scale is not a finite non-zero number; beta_a or beta_b not > 0 (NaN included); label_dropout outside [0, 1]. */
enum { TLD_DTYPE_U8 = 3 };
typedef struct tld_batch_source {
    const void* latents;
    const void* labels;
    const float* dequant_table;
    int64_t rows;
    int32_t latent_dtype, label_dtype;
    int32_t latent_elems, text_emb;
    float vae_scale;
} tld_batch_source;
TLD_API int tld_train_prepare_batch(tld_train* e, const tld_batch_source* src, const int64_t* idx, int32_t batch, uint64_t seed, uint64_t step,
                                    uint32_t replica, double beta_a, double beta_b, float label_dropout, float* x_noisy, float* noise_level,
                                    float* label, float* target, float* noise, double* noise_level64, uint8_t* mask, int32_t* bad_index_count,
                                    void* hip_stream);
/* tld_train_prepare_batch with the noise levels GIVEN (held-out evaluation at fixed levels).  noise_level_in: device fp64
 * [batch], 8-byte aligned: nl = noise_level_in[b], used as it is (a NaN propagates; the Python layer validates), the two Gamma draws of stream 1
 * are skipped and everything else is the plain entry's -- gather, Philox noise on stream 0, mask on stream 2 at label_dropout, the double mix,
 * noise_level = float(nl), the optional outputs (noise_level64 echoes the input).  NULL: exactly tld_train_prepare_batch, which is this call with
 * NULL.  The same refusals. */
TLD_API int tld_train_prepare_batch_at(tld_train* e, const tld_batch_source* src, const int64_t* idx, int32_t batch, uint64_t seed, uint64_t step,
                                       uint32_t replica, double beta_a, double beta_b, float label_dropout, float* x_noisy, float* noise_level,
                                       float* label, float* target, float* noise, double* noise_level64, uint8_t* mask, int32_t* bad_index_count,
                                       void* hip_stream, const double* noise_level_in);
/* ---- Held-out loss, per sample and by noise level ------------------------------------------------------------------
 * tld_train_forward_loss is the forward half of tld_train_forward_backward and nothing else: the same kernels in the same order (one internal
 * function under both entries) up to the per-row squared errors and the scalar loss, then tld_train_sample_loss on them.
 *   weights    flat fp32 device vector of tld_train_param_count elements (the EMA vector is the intended one): every parameter the forward reads
 *              comes from it, the bf16 / transposed operand copies included, which are rebuilt from it at the start of the call and marked stale
 *              at its end (the next training step rebuilds them from the bound parameters).  NULL or the bound params pointer: the bound parameters
 *   loss_out   device fp32 [1];  sample_loss_out  device fp64 [batch], may be NULL;  pred_out  device fp32 [batch, C, S, S], may be NULL (an
 *              engine-owned image of max_batch samples takes the prediction)
 * It never writes the bound gradient vector, invokes no callback and advances nothing; kernel launches only (a capturing stream is not refused).
 * TLD_ERR_INVALID: a NULL engine or required pointer, batch outside [1, max_batch]; TLD_ERR_STATE: before tld_train_bind, or with the stage hook
 * on (a debug call poisons the gradient vector).
 *
 * tld_train_sample_loss: out[b] = (sum_t row_sq[b rows_per_sample + t]) / elems_per_sample, summed in double in a fixed order (no atomics: bitwise
 * repeatable, and a sample's value does not depend on its position in the batch); a sample is non-finite exactly when one of its rows is.  out:
 * device fp64 [batch].  row_sq NULL: the engine's own row errors of its last forward, from either entry -- batch must be that call's batch (or that
 * of a forward captured into a graph, which replays out of the engine's sight), rows_per_sample / elems_per_sample are the engine's (tokens,
 * C S S) and the arguments are ignored; otherwise TLD_ERR_STATE.  row_sq non-NULL: any device fp32 array [batch, rows_per_sample]; e may be NULL.
 *
 * tld_train_loss_buckets accumulates into the caller-owned device fp64 vector state[2 n_buckets + 2] (all zeros = empty):
 *   [0, n) sum of the losses per bucket   [n, 2n) counts   [2n] sum of every accepted loss   [2n + 1] rejected samples
 * Sample b goes to bucket min(n - 1, floor((double)noise_level[b] * n)); a level outside [0, 1], NaN included, only increments the rejected
 * count; a non-finite loss is added as it is.  One workgroup, the owner of a cell adds b = 0 .. batch - 1 in order: after any sequence of calls the
 * state is what the serial loop gives on the host, bit for bit.  sample_loss device fp64 [batch], noise_level device fp32 [batch].
 * TLD_ERR_INVALID before any HIP call: a NULL pointer, state or sample_loss not 8-byte aligned, n_buckets outside [1, 256], batch < 1. */
TLD_API int tld_train_forward_loss(tld_train* e, const float* weights, const float* x_noisy, const float* noise_level, const float* label,
                                   const float* target, int32_t batch, float* loss_out, double* sample_loss_out, float* pred_out, void* hip_stream);
TLD_API int tld_train_sample_loss(tld_train* e, const float* row_sq, int32_t batch, int32_t rows_per_sample, int64_t elems_per_sample, double* out,
                                  void* hip_stream);
TLD_API int tld_train_loss_buckets(const double* sample_loss, const float* noise_level, int32_t batch, int32_t n_buckets, double* state,
                                   void* hip_stream);
/* Test hook: self-attention backward alone (head_dim 64; ntok a multiple of 16): qk [M, 2d] bf16 (q | k), vt [B, H, 64, ntok]
 * bf16, o [M, d] bf16 (forward output), g [M, d] fp32 (dL/dO) -> dqkv [M, 3d] bf16 (dq | dk | dv).  scratch: 2 * batch * heads * ntok floats
 * (row statistics between the two kernels of the ntok > 256 path; may be NULL otherwise).  Device pointers.
 * Sizes: every address is formed in 64 bits, so buffers beyond 4 GiB are accepted; TLD_ERR_INVALID before any launch only when
 * batch x heads x ceil(ntok / 32) workgroups pass 2^31 - 1. */
TLD_API int tld_debug_attention_bwd(const void* qk, const void* vt, const void* o, const float* g, void* dqkv, float* scratch, int32_t batch,
                                    int32_t ntok, int32_t heads, void* hip_stream);
/* Test hook: a weight gradient of the training step, dW[n_out, k_in] = dY^T X (dY [rows, n_out], X [rows, k_in] bf16 row-major; fp32 out):
 * both operands are read as they are (the contraction index is the row), split-K partial sums go through `slices` (slice_floats fp32).
 * n_out, k_in multiples of 256, rows a multiple of 64.  Device pointers.
 * Sizes: any number of rows (a 64-bit base per K-step); TLD_ERR_INVALID before any launch when n_out or k_in reaches 2^23 (a row of
 * either operand must stay below 2^24 bytes: the 24-bit multiply of the tile DMA). */
TLD_API int tld_debug_wgrad(const void* dy, const void* x, float* dw, float* slices, int64_t slice_floats, int32_t rows, int32_t n_out, int32_t k_in,
                            void* hip_stream);
/* Test / measurement hook: self-attention forward alone, softmax(q k^T / 8) v per head (head_dim 64; MHAttention.forward,
 * tld/transformer_blocks.py:31-48).  qk [batch * ntok, 2 d] bf16 (q | k), vt [batch, heads * 64, ntok] bf16 (V transposed per head),
 * att [batch * ntok, d] bf16 out, d = 64 heads.  iters launches back to back; *ms_per_launch (host pointer, may be NULL) receives the
 * HIP-event average.  Device pointers.
 * Sizes: every address is formed in 64 bits, so q | k beyond 4 GiB is accepted; TLD_ERR_INVALID before any launch when batch or heads
 * pass 65 535 at a token count whose kernel puts them on the grid's z and y axes (all but the multiples of 256 above 256), or when the
 * chunked kernel's workgroup count passes 2^31 - 1. */
TLD_API int tld_debug_attention_fwd(const void* qk, const void* vt, void* att, int32_t batch, int32_t ntok, int32_t heads, int32_t iters,
                                    float* ms_per_launch, void* hip_stream);
/* Test hook: the MLP's depthwise 3x3 convolution + GELU alone (nn.Conv2d(hid, hid, 3, padding=1, groups=hid) then nn.GELU() on the
 * "b (h w) c -> b c h w" view, tld/transformer_blocks.py:95-103) on channels-last tokens: in / out [batch, grid * grid, channels] bf16
 * (device), weight [channels, 9] and bias [channels] fp32 (HOST, the reference's conv.weight / conv.bias).  Runs the kernel the engine
 * would pick for that grid (whole-image / tiled / row-streaming).  channels % 64 == 0; grid a multiple of 4, as tld_engine_create has it
 * (any other side is refused with the engine's words, "token count ... unsupported"): the partial last 16 x 16 tiles of 20, 24, 28 ... included.
 * Sizes: the row-streaming kernel (grids that are multiples of 32) writes through 32-bit byte offsets: batch x grid^2 x channels x 2 B
 * must stay below 4 GiB, else TLD_ERR_INVALID before any allocation or launch, with the largest batch that fits.  The whole-image and
 * tiled kernels address in 64 bits and accept larger buffers (up to 2^31 - 1 workgroups). */
TLD_API int tld_debug_dwconv_gelu(const void* in_bf16, const float* weight_host, const float* bias_host, void* out_bf16, int32_t batch,
                                  int32_t grid, int32_t channels, void* hip_stream);
/* The training step's stages (the stage hook above).  With debug on, one
 * tld_train_forward_backward call
 *   - first fills every engine-owned activation / statistics / scratch / partial-sum buffer and the bound gradient vector with 0xFF bytes
 *     (NaN in bf16 and fp32), so that a kernel that stores nothing, or too few rows, shows as NaN instead of the previous call's values;
 *   - keeps what the backward overwrites.
 *     Snapshot memory (for max_batch samples) is allocated by set_debug(1), which fails if it cannot be had, and freed by set_debug(0) / destroy;
 *     create allocates none, a step allocates none;
 *   - records which launch path every size-dependent dispatch took (tld_train_debug_paths).
 * With debug off nothing is launched, copied or allocated for the hook.  A debug call on a capturing stream is refused (TLD_ERR_STATE).
 * Each path bit is set inside the branch that launches the kernel (the attention bits by launch_attention_bwd itself): the launch sites RECORD the
 * mask.  The plan of the step (csrc/tld_train_plan.h: train_step_plan(...).paths, a pure host function of the configuration, the batch, the CU count and
 * TLD_TRAIN_TN_WGRAD) PREDICTS it; tests hold the recorded mask of every case against the prediction.
 *
 * Stage names (i = block index; M = batch * tokens; every stage is read back as fp32 with its logical shape):
 *   saved forward tensors, read in place:  blk<i>.{x1 a1 qk vt att x2 a2 qc cr x3 a3 h hc o} (bf16; hc = GELU'(pre-activation) as stored),
 *     blk<i>.{st1 st2 st3} [M, 2] (mean, rstd), blk<i>.p0 [M, H], blk<i>.kvc [2 batch, 2 d], sinb h1 g1v ycat y yst, p16 p16n est1 e est2,
 *     xfin, dout, row_loss; the bf16 GEMM operand copies blk<i>.{wqkv wq wup wdown} and their transposes blk<i>.{wqkv_t wq_t wup_t wdown_t};
 *   copied:  blk<i>.gl (GELU output, before the backward reuses its buffer), gx.tail, gxb.tail, and per block
 *     gx.in (= the gradient entering the block), dg, dhc (unfused depthwise backward only), dh, da3, gx.ln3, dqc, dkv, da2, gx.ln2,
 *     dqkv, da1, gx.ln1, gxb.ln1 (blocks > 0), each under blk<i>.; then dy, de, dpn, dp16, dycat, dg1.
 * Launch-path bits of tld_train_debug_paths (bit number : path):
 *    0 resid_ln q4<1>   1 q4<2>   2 q4<3>   3 q4<4>   4 resid_ln generic        5 ln_bwd q4<1>   6 q4<2>   7 q4<3>   8 ln_bwd generic
 *    9 embed LDS<1>    10 LDS<2>  11 LDS<3>  12 LDS<4>  13 embed plain           14 tail_dx4<16>  15 <32>   16 <64>   17 tail_dx generic
 *   18 tall_dw_cols    19 tall_dw_partial             20 colsum4   21 colsum     22 depthwise backward fused   23 unfused
 *   24 wgrad_tn        25 transposing wgrad, sk == 1  26 sk > 1    27 zero-padded (M % 64 != 0)
 *   28 attention backward one kernel   29 two kernels   30 masked (token count not a multiple of the block) */
#define TLD_TRAIN_PATH_BITS 31
TLD_API int tld_train_set_debug(tld_train* e, int32_t enable);
/* shape_out may be NULL; host_out NULL: only the shape. */
TLD_API int tld_train_read_stage(tld_train* e, const char* name, float* host_out, int64_t numel, int64_t* shape_out);
/* mask of the launch paths the last debug call took */
TLD_API int tld_train_debug_paths(tld_train* e, uint64_t* mask);
TLD_API int tld_train_destroy(tld_train* e);

/* ---- Distribution metrics on embedding banks ---------------------------------------------------------------------------
 * The reference leaves its FID script as a TODO (README.md:237).  These three kernels give the two statistics such a script takes -- the moments of a
 * Frechet distance and the pair sums of a kernel MMD (CMMD: Jayasumana et al. 2024) -- over embeddings that stay on the device.
 *
 * A bank is a plain device fp32 matrix [capacity, pitch]; pitch = dim rounded up to a multiple of 32, pad columns zero; dim in [1, 4096].  Every
 * entry point takes device pointers, enqueues on hip_stream without synchronising, uses no atomic on a value and repeats bitwise.
 *
 * tld_feat_append: rows [used, used + rows) of the bank from src [rows, dim] (contiguous; fp32, bf16 or fp16 by src_dtype).  normalize = 1: each row is
 * divided by its L2 norm; the squares are added in double in ascending column order, the quotient is formed in double and rounded to fp32 once.  A row
 * with a non-finite value (or, with normalize = 1, norm 0) is stored as zeros and adds one to *bad_count (device int32; the caller zeroes it).
 * Refused (TLD_ERR_INVALID, before any HIP call): null pointers, dim, pitch, src_dtype, rows < 1, rows that do not fit [used, capacity). */
TLD_API int tld_feat_append(float* bank, int64_t capacity, int64_t used, int32_t dim, int32_t pitch, const void* src, int32_t src_dtype, int64_t rows,
                            int32_t normalize, int32_t* bad_count, void* hip_stream);
/* mean [dim] and cov [dim, dim] (double, device) of rows [0, n) of the bank: numpy.mean(axis=0) and numpy.cov(rowvar=False) -- ddof = 1, two passes,
 * centred in double, every sum in a fixed order; cov is symmetric bit for bit.  Refused: null pointers, dim, pitch, n < 2. */
TLD_API int tld_feat_moments(const float* bank, int64_t n, int32_t dim, int32_t pitch, double* mean, double* cov, void* hip_stream);
/* Doubles of `partials` a tld_feat_kernel_sum call of these sizes needs (one per 128 x 128 tile of its plan); 0 for sizes it refuses.  Needs no GPU. */
TLD_API int64_t tld_feat_kernel_sum_partials(int64_t na, int64_t nb, int32_t same);
/* out[0] = sum_{i < na, j < nb} expm1(-gamma d2_ij), d2_ij = max(0, |a_i|^2 + |b_j|^2 - 2 a_i . b_j), over rows [0, na) of a and [0, nb) of b (banks of one
 * dim and pitch; 16-byte aligned).  k - 1, not k: the ones cancel exactly in every MMD estimator.  same = 1: b is a, the terms i == j are the constant
 * 0, and only tiles on or above the diagonal run.  Dot products on the fp32 MFMA, row norms from an fp32 fmaf chain in the same order, expm1f, then
 * double.  partials [n_partials >= tld_feat_kernel_sum_partials(na, nb, same)] is workspace; nothing outside rows < na / < nb is read.
 * Refused: null pointers, dim, pitch, na or nb < 1, same = 1 with na != nb or a != b, a negative or non-finite gamma, too few partials. */
TLD_API int tld_feat_kernel_sum(const float* a, int64_t na, const float* b, int64_t nb, int32_t dim, int32_t pitch, double gamma, int32_t same,
                                double* partials, int64_t n_partials, double* out, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* TLD_HIP_H */

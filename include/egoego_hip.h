/*
 * egoego_hip.h — C ABI of libegoego_hip.so: the MI355X (gfx950) implementation of EgoEgo's
 * stage-2 conditional motion-diffusion sampling step.
 *
 * The reference (lijiaman/egoego_release) is pure Python/PyTorch and has no native interface;
 * each entry point below replaces the PyTorch op sequence of the cited reference function.
 * Paths are relative to the reference root:
 *   M  = egoego/model/transformer_cond_diffusion_model.py
 *   TM = egoego/model/transformer_module.py
 *
 * Conventions
 *   - every pointer named d_* is a DEVICE pointer owned by the caller (PyTorch allocates all I/O
 *     tensors and the workspace); the library never frees or retains caller memory except the
 *     workspace during a call, and launches only on `stream` (a hipStream_t passed as void*;
 *     NULL = the legacy default stream).
 *   - synchronisation: the SAMPLING entry points (egoego_denoise, _p_sample, _sample_loop, _ddim_loop,
 *     _rot6d_to_matrix, _convert_model_res, _window_condition, _window_prefix, _debug_stage) only enqueue
 *     work and return; they never wait for the stream.  (egoego_ddim_loop stages its step table in a pinned
 *     slot and waits, at most, for the copy of the call four calls earlier; egoego_sample_loop drains the DEVICE
 *     once if a context has seen more than eight distinct step shapes and must evict a captured graph.)
 *     The SETUP entry points egoego_load_weights and egoego_load_schedule DO call hipStreamSynchronize(stream)
 *     (host staging buffers; a re-load first waits for work that still reads the old weights), and
 *     egoego_profile_end waits for its events.
 *   - `stream` must NOT be in capture mode (torch.cuda.graph / hipStreamBeginCapture by the caller):
 *     the multi-step loops capture their own per-step hipGraph on a private stream (relaxed mode) and launch
 *     graphs on `stream`, and the setup calls synchronise.  egoego_denoise / egoego_p_sample are plain kernel
 *     launches and can be captured by the caller once the context has run that shape (first use sets kernel
 *     attributes).
 *   - pose tensors are fp32, contiguous, [B][T][d_feats]; timesteps are int64 [B] (torch.long).
 *   - return value: 0 = ok; negative = error (EGOEGO_E_*); egoego_last_error() describes the last
 *     failure on the calling thread.
 *   - any number of contexts may live on one device (the Python side holds up to three at a time: the plan's, its unshifted
 *     twin for padding-mask calls, and the split-bf16 reference of a pack-time measurement); a context is not thread-safe.
 *     A context and each workspace are SINGLE-STREAM objects: the
 *     captured step graphs are shared by every call of a shape, and the per-workspace step state (timestep counters, the
 *     caller's buffer pointers, the Philox key) is rewritten by every loop call — two streams driving one workspace or one
 *     context concurrently race silently.  Use one context + workspace per stream.
 *   - workspace contents: what a workspace holds ON ENTRY is irrelevant to every result of every entry point that takes one
 *     (egoego_denoise / _p_sample / _sample_loop / _ddim_loop and their _ragged forms, egoego_debug_stage, egoego_s1_encode,
 *     egoego_flow_features, egoego_body_forward, egoego_win_stats, egoego_amass_floor_contacts): any bytes will do — zeros, NaN or infinity patterns, what an
 *     earlier call of another shape left — and the same call gives the same bits.  No value that a kernel uses as an index, a
 *     count, a timestep or an address is read before the same call has written it; stale values are only ever read as DATA of
 *     rows, keys or frames that are never stored (DESIGN.md 4a lists every region with its writer).  A workspace needs no
 *     clearing before use and may be shared by calls of different shapes, one after the other.
 *     The ONE exception is the stage-2 outlier monitor (StepState::ln_max, the first bytes of a stage-2 workspace): it
 *     accumulates over calls by design and is read only by egoego_outlier_stats.  Establish it with
 *     egoego_outlier_stats(ctx, B, T, ws, bytes, NULL, 0, 1, stream) on a workspace that is new or whose bytes were overwritten
 *     from outside (engine.py does for each buffer it allocates); no sampling result depends on it.
 */
#ifndef EGOEGO_HIP_H
#define EGOEGO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EGOEGO_ABI_VERSION 8 /* 5: EGOEGO_FLAG_FC24; 6: EGOEGO_FLAG_FFN16; 7: stage 1 (egoego_s1_*); 8: flow CNN (egoego_flow_*); the body model (egoego_body_*), the evaluation (egoego_eval_*), the motion windows (egoego_win_*), the ragged sampling entry points (egoego_*_ragged) the AMASS preprocessing (egoego_amass_*) the stage-2 training step (egoego_train_*) and stage 1's alignment and score (egoego_s1_gravity_align, egoego_s1_head_pose_metrics) were added under 8: purely additive, no existing entry changed */

enum {
    EGOEGO_OK = 0,
    EGOEGO_E_INVALID = -1,   /* bad argument / unsupported shape */
    EGOEGO_E_HIP = -2,       /* a HIP runtime call failed */
    EGOEGO_E_STATE = -3,     /* weights or schedule not loaded yet */
    EGOEGO_E_WORKSPACE = -4  /* workspace too small or misaligned */
};

enum { EGOEGO_PRED_NOISE = 0, EGOEGO_PRED_X0 = 1 };        /* M:235-240 */
enum { EGOEGO_NOISE_INJECTED = 0, EGOEGO_NOISE_PHILOX = 1, EGOEGO_NOISE_NONE = 2 };
/* operand precision of every contraction: 3 = split-bf16 (hi*hi + lo*hi + hi*lo, fp32 accumulate;
 * meets the 1e-3 parity bar), 1 = plain bf16 operands (fast, does NOT meet it; reported only),
 * 8 = the contractions whose input rows have one natural scale — the Q/K/V projections, QK^T, PV and the two FFN convs —
 * computed from two int8 slices per operand (three int8 MFMAs per product, int32 accumulate; same parity bar); embed, fc and
 * linear_out stay split-bf16.
 * 9 = 8 with the attention output projection (fc) and linear_out on int8 slices as well: the attention kernels hand O over as
 * int8 rows with one scale per row and head, fc runs one exact integer chain per head, and every activation that crosses memory
 * between the kernels of a step is an int8 row (the residual stream included).  Same parity bar, about twice the error of 8
 * (~3e-4 against ~1.3e-4 on one forward), about 30 % less time per step at every batch size (8: +40 %, 3: +80-90 % over 9),
 * and more sensitive to outlier-heavy checkpoints
 * (LayerNorm gains far above the rest: DESIGN.md 3c). */
enum { EGOEGO_PREC_BF16X3 = 3, EGOEGO_PREC_BF16X1 = 1, EGOEGO_PREC_I8X3 = 8, EGOEGO_PREC_I8X3_FC = 9 };

typedef struct egoego_ctx egoego_ctx;

/* Shapes of TransformerDiffusionModel (M:75-116) / CondGaussianDiffusion.__init__ (M:144-161). */
typedef struct {
    int32_t d_feats;        /* 198 */
    int32_t d_model;        /* 512 (only value supported) */
    int32_t n_head;         /* 4 */
    int32_t n_dec_layers;   /* 4 */
    int32_t d_k;            /* 256 (only value supported) */
    int32_t d_v;            /* 256 (only value supported) */
    int32_t max_timesteps;  /* window + 1; the position table has max_timesteps + 1 rows (TM:180-182) */
    int32_t num_timesteps;  /* diffusion steps S, 1000 */
    int32_t objective;      /* EGOEGO_PRED_X0 | EGOEGO_PRED_NOISE */
    int32_t precision;      /* EGOEGO_PREC_BF16X3 | EGOEGO_PREC_BF16X1 | EGOEGO_PREC_I8X3 | EGOEGO_PREC_I8X3_FC */
    int32_t flags;          /* EGOEGO_FLAG_* (0 = defaults) */
} egoego_config;

/* egoego_sample_loop / egoego_ddim_loop capture one diffusion step into a hipGraph and replay it for the rest of the
 * chain (the timestep lives in device memory); this flag launches every kernel of every step individually instead. */
enum { EGOEGO_FLAG_NO_GRAPH = 1 };
/* EGOEGO_PREC_I8X3_FC only: fc's weights (self_attn.fc, TM:55) as THREE int8 slices — w = scale * (q16 + w3 / 256): a second
 * contraction per feature pass adds the third slice's products (about +10 % time per step).  On a trained checkpoint fc on the
 * 16-bit grid is what separates precision 9 from 8 at the end of a 1000-step chain; the Python layer's "auto"
 * tries this form before falling back to precision 8.  Hand the fc weights over UNROUNDED when it is set. */
enum { EGOEGO_FLAG_FC24 = 2 };
/* EGOEGO_PREC_I8X3 only: the FFN contractions (pos_ffn.w_1 / w_2, TM:102-103) on split-bf16 like fc — int8 slices are then confined to
 * the attention layer (Q/K/V projections, QK^T, PV).  Fewer fixed-point sites at the time per step of precision 8 on large batches (its
 * int8-FFN tail is no faster than the split-bf16 one there); the Python layer's "auto" tries this form after "8 prepared".
 * Hand the FFN weights over UNROUNDED when it is set. */
enum { EGOEGO_FLAG_FFN16 = 4 };

/* fp32 device tensors in the reference checkpoint layout, contiguous. */
typedef struct {
    const float* w_q; const float* b_q;      /* self_attn.w_q  (H*dk, 512), (H*dk)   TM:45 */
    const float* w_k; const float* b_k;      /* self_attn.w_k                         TM:46 */
    const float* w_v; const float* b_v;      /* self_attn.w_v  (H*dv, 512)            TM:47 */
    const float* w_fc; const float* b_fc;    /* self_attn.fc   (512, H*dv)            TM:55 */
    const float* ln1_g; const float* ln1_b;  /* self_attn.layer_norm                  TM:57 */
    const float* w_1; const float* b_1;      /* pos_ffn.w_1    (512, 512, 1)          TM:102 */
    const float* w_2; const float* b_2;      /* pos_ffn.w_2    (512, 512, 1)          TM:103 */
    const float* ln2_g; const float* ln2_b;  /* pos_ffn.layer_norm                    TM:104 */
} egoego_layer_weights;

typedef struct {
    const float* start_conv_w; const float* start_conv_b;  /* (512, 2*d_feats, 1), (512)   TM:179 */
    const float* position_vec;                              /* (max_timesteps+1, 512)       TM:180 */
    const float* linear_out_w; const float* linear_out_b;  /* (d_feats, 512), (d_feats)    M:102 */
    const float* time_mlp1_w; const float* time_mlp1_b;    /* (256, 64), (256)             M:113 */
    const float* time_mlp3_w; const float* time_mlp3_b;    /* (512, 256), (512)            M:115 */
    const egoego_layer_weights* layers;                     /* HOST array of n_dec_layers entries */
} egoego_weights;

/* fp32 HOST arrays of num_timesteps entries: the buffers registered at M:191-211. */
typedef struct {
    const float* posterior_mean_coef1;
    const float* posterior_mean_coef2;
    const float* posterior_log_variance_clipped;
    const float* sqrt_recip_alphas_cumprod;
    const float* sqrt_recipm1_alphas_cumprod;
    const float* alphas_cumprod;   /* used by the DDIM sampler only */
} egoego_schedule;

int egoego_abi_version(void);
const char* egoego_last_error(void);

/* Replaces: module construction + .to(device) (M:144-214). */
int egoego_ctx_create(const egoego_config* cfg, int device, egoego_ctx** out);
void egoego_ctx_destroy(egoego_ctx* ctx);

/* Replaces: load_state_dict (trainer_amass_cond_motion_diffusion.py:116-122).  Packs the fp32
 * tensors into the library's split-bf16 fragment-tiled copies and precomputes the time-token
 * table (M:61-73, 111-116).  The caller keeps its originals and may free them after the stream
 * has drained. */
int egoego_load_weights(egoego_ctx* ctx, const egoego_weights* w, void* stream);
int egoego_load_schedule(egoego_ctx* ctx, const egoego_schedule* s, void* stream);

/* Bytes of scratch a call with batch B and window length T needs (256-byte aligned base).
 * Returns 0 (egoego_last_error() says why) for shapes no call accepts: T + 1 > 224 or > max_timesteps, or more than
 * 2^20 padded rows per call (B * 32 * ceil((T + 1) / 32); T + 1 in 129..224 pads to 224): B <= 8192 at T = 120,
 * B <= 4681 at T = 196 — split larger batches, windows are independent. */
size_t egoego_workspace_bytes(const egoego_ctx* ctx, int B, int T);

/* Replaces TransformerDiffusionModel.forward on cat(x, x_cond) (M:118-141, 232-233):
 * d_out[B][T][D] = denoiser(cat(x, x_cond), t).  d_row_mask: optional fp32 [B][T+1] padding mask
 * (1 keep / 0 zero the row after attention and after the FFN, TM:135,139), NULL = all ones. */
int egoego_denoise(egoego_ctx* ctx, const float* d_x, const float* d_x_cond, const int64_t* d_t,
                   const float* d_row_mask, float* d_out, int B, int T,
                   void* d_workspace, size_t workspace_bytes, void* stream);

/* Replaces CondGaussianDiffusion.p_sample (M:248-256): x <- posterior_mean(clamp(x0_pred), x, t)
 * + 1[t>0] * exp(0.5*logvar[t]) * noise, in place.  d_noise: fp32 [B][T][D] (the caller's
 * randn_like draw) or NULL with noise_mode PHILOX/NONE.  clip_denoised mirrors M:242-243. */
int egoego_p_sample(egoego_ctx* ctx, float* d_x, const float* d_x_cond, const int64_t* d_t,
                    const float* d_row_mask, const float* d_noise, int noise_mode,
                    uint64_t seed, int64_t window_offset, int clip_denoised, int B, int T,
                    void* d_workspace, size_t workspace_bytes, void* stream);

/* Replaces the body of p_sample_loop (M:267-268) and of the sliding-window loop (M:392-397):
 * for i = t_start .. t_start-n_steps+1: x <- p_sample(x, i, x_cond, padding_mask); optionally overwrite the first
 * prefix_len frames of every window with d_prefix[B][prefix_len][D] after every step (M:395-397).
 * d_row_mask: the padding mask p_sample_loop hands to every step (M:259,268), fp32 [B][T+1] as for
 * egoego_denoise, or NULL.
 * Noise per step: EGOEGO_NOISE_INJECTED reads d_noise[step][B][T][D] (step 0 = first executed
 * step); EGOEGO_NOISE_PHILOX draws N(0,1) in-kernel from Philox4x32-10 keyed by
 * (seed; window_offset + b, timestep, frame, feature) so results do not depend on how windows are
 * sharded over GPUs. */
int egoego_sample_loop(egoego_ctx* ctx, float* d_x, const float* d_x_cond, int t_start, int n_steps,
                       const float* d_noise, int noise_mode, uint64_t seed, int64_t window_offset,
                       const float* d_prefix, int prefix_len, const float* d_row_mask, int B, int T,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* RAGGED batches: windows of different lengths in one call.  The three entry points below are egoego_denoise, egoego_p_sample
 * and egoego_sample_loop with two more arguments (the ABI version stays 8: purely additive):
 *   d_lengths     int32 DEVICE array [B], each 1..T: the frames of window b.  Window b then attends over its time token and its
 *                 first d_lengths[b] frames only — what the reference computes when it calls the denoiser on a window of that
 *                 length (M:355-356) — where a padding mask (d_row_mask: still available, and independent) only zeroes sublayer
 *                 outputs while the padded frames keep acting as keys (TM:135,139).  NULL: every window has T frames.
 *   d_window_ids  int64 DEVICE array [B]: window b draws the Philox stream of id d_window_ids[b], so a compacted or reordered set
 *                 of windows keeps each window's own noise.  NULL: window_offset + b.
 * The values are the caller's responsibility (the Python layer validates them, and that prefix_len <= min(lengths)); both arrays
 * must stay valid until the call's work on `stream` is done.
 * What a ragged call guarantees: the rows of a window up to its length depend on that window's own rows and its own length only —
 * they are bit-identical with the window alone in the batch, at any position of it, among any other lengths and for any ids of
 * the other windows; with every length equal to T (and ids window_offset + b) they are the bits of the uniform entry point.  The
 * rows PAST a window's length are unspecified but finite: they are computed like any others (no row mask is implied), attend over
 * the window's valid keys and stay inside the per-step clamp; the outlier monitor records them as computed.  Tile and form
 * selection is that of the padded (B, T): a short window costs what a full one does.
 * One captured step serves every ragged call of a shape on a workspace (the arrays are step state, never graph arguments); uniform
 * and ragged calls of the same shape keep separate graphs (they launch different kernel instantiations).
 * The strided sampler has its ragged form too (egoego_ddim_loop_ragged, below).  NOT ragged: egoego_debug_stage takes one T for
 * the whole batch. */
int egoego_denoise_ragged(egoego_ctx* ctx, const float* d_x, const float* d_x_cond, const int64_t* d_t,
                          const float* d_row_mask, const int32_t* d_lengths, float* d_out, int B, int T,
                          void* d_workspace, size_t workspace_bytes, void* stream);
int egoego_p_sample_ragged(egoego_ctx* ctx, float* d_x, const float* d_x_cond, const int64_t* d_t,
                           const float* d_row_mask, const int32_t* d_lengths, const int64_t* d_window_ids,
                           const float* d_noise, int noise_mode, uint64_t seed, int64_t window_offset, int clip_denoised,
                           int B, int T, void* d_workspace, size_t workspace_bytes, void* stream);
int egoego_sample_loop_ragged(egoego_ctx* ctx, float* d_x, const float* d_x_cond, int t_start, int n_steps,
                              const float* d_noise, int noise_mode, uint64_t seed, int64_t window_offset,
                              const float* d_prefix, int prefix_len, const float* d_row_mask,
                              const int32_t* d_lengths, const int64_t* d_window_ids, int B, int T,
                              void* d_workspace, size_t workspace_bytes, void* stream);

/* DDIM sampler (Song et al. 2021) on a strided subsequence of timesteps.  NOT in the reference —
 * no oracle from the reference exists for it.  timesteps_host: HOST int32 array of n strictly descending timesteps.
 * eta in [0, 1]: 0 = deterministic; 1 on the FULL timestep list is the ancestral DDPM chain of egoego_sample_loop
 * (sigma_t^2 = posterior variance), which is how the sampler is tied to the reference's chain (tests).  Noise for
 * eta > 0 as for egoego_sample_loop (d_noise[step][B][T][D] or Philox keyed by (seed; window_offset + b, timestep, ..)). */
int egoego_ddim_loop(egoego_ctx* ctx, float* d_x, const float* d_x_cond, const int32_t* timesteps_host, int n,
                     float eta, const float* d_noise, int noise_mode, uint64_t seed, int64_t window_offset,
                     int B, int T, void* d_workspace, size_t workspace_bytes, void* stream);

/* egoego_ddim_loop through the sliding-window harnesses: the same chain plus the five arguments egoego_sample_loop_ragged adds to
 * egoego_sample_loop, with the same meaning and lifetime rules (the ABI version stays 8: purely additive).
 *   d_prefix / prefix_len  the first prefix_len frames of every window are overwritten with d_prefix[B][prefix_len][D] after EVERY
 *                          step, the last included (M:395-397).  The prefix is imposed clean, as the reference does for its own
 *                          chain: no noise-matched in-painting.  prefix_len in 1..T when d_prefix is given; NULL: none.
 *   d_row_mask             fp32 [B][T+1] padding mask handed to every step, or NULL.
 *   d_lengths, d_window_ids  as for the ragged entry points above: DEVICE arrays read through the step state, never graph
 *                          arguments, so one captured step serves every later call of that (B, T, noise mode, prefix_len, mask,
 *                          ragged) shape on a workspace, whatever its timestep list, arrays and buffers.
 * Per-step Philox draws stay keyed by the actual timestep: an eta > 0 strided chain draws, at timestep t, the stream the ancestral
 * chain draws there.  With d_prefix, d_row_mask, d_lengths and d_window_ids all NULL this is egoego_ddim_loop, bit for bit. */
int egoego_ddim_loop_ragged(egoego_ctx* ctx, float* d_x, const float* d_x_cond, const int32_t* timesteps_host, int n,
                            float eta, const float* d_noise, int noise_mode, uint64_t seed, int64_t window_offset,
                            const float* d_prefix, int prefix_len, const float* d_row_mask,
                            const int32_t* d_lengths, const int64_t* d_window_ids, int B, int T,
                            void* d_workspace, size_t workspace_bytes, void* stream);

/* Replaces pytorch3d.transforms.rotation_6d_to_matrix at M:493: d_in [n][6] -> d_out [n][3][3]. */
int egoego_rot6d_to_matrix(const float* d_in, float* d_out, int64_t n, void* stream);

/* Replaces the post-loop conversion chain of one batch of windows: convert_model_res_to_data (M:469-525) with
 * quat_ik (amass_diffusion_dataset.py:109-125) and the pytorch3d calls inside them (6D -> matrix -> quaternion,
 * un-canonicalise, global -> local rotations, -> axis-angle; de-normalise and rotate the root / head positions).
 *   d_x [B][T][198] normalised model output; d_rec_quat [B][4] (w,x,y,z) = recover_rot_quat (M:470);
 *   d_jpos_min / d_jpos_max [66] = ds.global_jpos_min/max (amass_diffusion_dataset.py:379-392);
 *   parents_host[22]: HOST array, parents_host[j] < j for j > 0 (the SMPL-H kintree, an input: SURVEY.md §8f #1);
 *   d_aa [B][T][22][3] local axis-angle, d_root [B][T][3], d_head [B][T][3] (joint head_idx). */
int egoego_convert_model_res(const float* d_x, const float* d_rec_quat, const float* d_jpos_min, const float* d_jpos_max,
                             const int32_t* parents_host, int head_idx, int B, int T, float* d_aa, float* d_root, float* d_head,
                             void* stream);

/* The head condition of one sliding window (M:355-378): d_head_jpos [B][Tw][3] and d_head_jquat [B][Tw][4] (w,x,y,z) are
 * canonicalised about the first frame's heading (rotate_at_frame, lafan1/utils.py:111-137; its xy moved to the origin) and
 * written into an otherwise zero d_x_start [B][Tw][198] (position dims 3*head_idx.., 6D dims 66 + 6*head_idx..), joint
 * positions min/max-normalised; d_recover_quat [B][4] receives the un-canonicalising rotation (recover_rot_quat of M:470). */
int egoego_window_condition(const float* d_head_jpos, const float* d_head_jquat, const float* d_jpos_min, const float* d_jpos_max,
                            int head_idx, int B, int Tw, float* d_x_start, float* d_recover_quat, void* stream);

/* The condition of the next sliding window (M:399-467) from the current window's converted output: fk_smpl
 * (amass_diffusion_dataset.py:265-293) over the last n_last frames, rotate_at_frame (lafan1/utils.py:111-137) about
 * their first frame's head heading, joint positions min/max-normalised (amass_diffusion_dataset.py:379-392), rotations
 * as 6D.  d_aa [B][Tw][22][3], d_root [B][Tw][3] (egoego_convert_model_res' outputs, root already shifted),
 * d_rest_offsets [22][3] = ds.rest_human_offsets, parents_host[22] as above -> d_prefix [B][n_last][198], the
 * `d_prefix` argument of egoego_sample_loop for the next window. */
int egoego_window_prefix(const float* d_aa, const float* d_root, const float* d_rest_offsets, const float* d_jpos_min,
                         const float* d_jpos_max, const int32_t* parents_host, int head_idx, int B, int Tw, int n_last,
                         float* d_prefix, void* stream);

/* Per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
 * kernel_id: EGOEGO_K_*.  begin() arms event pairs around every launch of that kernel;
 * end() synchronises the stream's events and returns the mean duration and launch count. */
enum { EGOEGO_K_QKV = 0, EGOEGO_K_ATTN = 1, EGOEGO_K_FC_LN = 2, EGOEGO_K_FFN1 = 3, EGOEGO_K_FFN2_LN = 4,
       EGOEGO_K_EMBED = 5, EGOEGO_K_OUT = 6, EGOEGO_K_COUNT = 7 };
int egoego_profile_begin(egoego_ctx* ctx, int kernel_id);
int egoego_profile_end(egoego_ctx* ctx, double* mean_us, int* launches);
/* The kernel variant the launch site `kernel_id` of a step last dispatched to in this context (the library picks tile shapes and
 * fused / split forms by batch size, window length and precision): e.g. "attn_layer_i8w_kernel", "tail_kernel<1,true,true,true,4,true>".
 * "" before the first step.  What bench.py names its roofline kernels from (no dispatch logic outside the library). */
const char* egoego_last_kernel_name(const egoego_ctx* ctx, int kernel_id);

/* Outlier monitor of the int8-slice precisions (8, 9).  Those keep ONE scale per activation row (16-bit fixed point): a row whose
 * largest entry is far above the rest costs every other entry of the row that many bits.  Every LayerNorm epilogue that
 * quantises its rows records the largest |value| it has seen (one atomicMax per workgroup into the workspace's step state).
 * Only those record, so the sites a call fills depend on the form:
 *   precision 8, and precision 9 at T + 1 <= 64 (it runs precision 8's kernels there): LayerNorm-1 of every layer, LayerNorm-2 of
 *     every layer but the last (linear_out reads the last layer's split-bf16 rows);
 *   precision 8 + EGOEGO_FLAG_FFN16: LayerNorm-2 of every layer but the last, no LayerNorm-1 (the FFN reads split-bf16 rows);
 *   precision 9 at T + 1 >= 65, with EGOEGO_FLAG_FC24 or not: both LayerNorms of every layer;
 *   precisions 3 / 1, and layers >= 8: nothing.
 * Every row of the B windows is recorded: with a row mask each window's padding rows (T + 1 .. Lr - 1) are zero, without one they
 * are recorded as computed.  A ragged call (egoego_*_ragged) implies no row mask: the rows past a window's own length are computed
 * like any others — over the window's valid keys only, so finite and inside the per-step clamp — and recorded as computed.
 * Only the rows that pad the call to whole token blocks are not.  Weights packed from a mean-shifted
 * state dict record the shifted rows (the LayerNorm output minus the per-feature shift).
 * host_out[2 * layer + k] (k = 0: self_attn.layer_norm, k = 1: pos_ffn.layer_norm; n_out <= 16 entries, 0 = nothing recorded)
 * receives the maxima accumulated by every call on this workspace since the last reset; reset != 0 clears them afterwards.
 * Divide by the rms of the LayerNorm's (gain, bias) to get the row's crest factor — what model.py's runtime guard compares
 * with its measured limit.  SYNCHRONISES `stream` when n_out > 0.  A freshly allocated workspace holds
 * undefined values: call once with n_out = 0, reset = 1 (engine.py does) before relying on the maxima. */
int egoego_outlier_stats(egoego_ctx* ctx, int B, int T, void* d_workspace, size_t workspace_bytes, float* host_out, int n_out,
                         int reset, void* stream);

/* Test/debug only: run the denoiser up to and including `stage` of decoder layer `layer` and
 * return that intermediate as fp32 row-major.  Stages: EGOEGO_DBG_*.  Output shapes:
 *   EMBED/ATTN_LN/FFN_HIDDEN/LAYER_OUT: [B][T+1][512]; Q/K/V: [B][H][T+1][256]; ATTN_OUT: [B][T+1][H*256]. */
enum { EGOEGO_DBG_EMBED = 0, EGOEGO_DBG_Q = 1, EGOEGO_DBG_K = 2, EGOEGO_DBG_V = 3, EGOEGO_DBG_ATTN_OUT = 4,
       EGOEGO_DBG_ATTN_LN = 5, EGOEGO_DBG_FFN_HIDDEN = 6, EGOEGO_DBG_LAYER_OUT = 7 };
int egoego_debug_stage(egoego_ctx* ctx, const float* d_x, const float* d_x_cond, const int64_t* d_t,
                       const float* d_row_mask, int layer, int stage, float* d_out, int B, int T,
                       void* d_workspace, size_t workspace_bytes, void* stream);

/* ==================================================================================================================
 * Stage 1: the head-pose estimators HeadNet (HeadFormer, egoego/model/head_estimation_transformer.py = HE) and GravityNet
 * (HeadNormalFormer, egoego/model/head_normal_estimation_transformer.py = HN) with precomputed optical-flow features
 * (input_of_feats).  Both are the TM Decoder at d_model 256 (use_full_attention=True) plus ReLU MLP heads; every contraction
 * is split-bf16 (three bf16 MFMAs, fp32 accumulate).  A stage-1 context is separate from the stage-2 one; the conventions above
 * (device pointers, caller's stream, return codes) hold, and egoego_s1_last_error() describes the last stage-1 failure.
 *
 * Windows: a call runs W independent windows of `window` tokens each.  d_feats is [W][window][d_feats] fp32 (tokens past
 * valid[w] are ignored and read as zero rows, as the reference's zero padding); d_valid is int32 [W], 0..window (more counts as window).  A padded
 * token is NOT masked as a key (TM:126-141): it only has its sublayer outputs zeroed.
 * ================================================================================================================== */
enum { EGOEGO_S1_HEADNET = 0, EGOEGO_S1_GRAVITYNET = 1 };

typedef struct egoego_s1_ctx egoego_s1_ctx;

typedef struct {
    int32_t kind;          /* EGOEGO_S1_HEADNET | EGOEGO_S1_GRAVITYNET */
    int32_t d_feats;       /* 512 (HeadNet) / 18 (GravityNet); 1..1024 accepted */
    int32_t d_model;       /* 256 (only value supported) */
    int32_t n_head;        /* n_head * d_k == n_head * d_v == 1024 (only value supported) */
    int32_t n_dec_layers;  /* 1..8 */
    int32_t d_k;
    int32_t d_v;
    int32_t window;        /* 1..128: tokens per window; the position table has window + 1 rows (TM:180-182) */
} egoego_s1_config;

/* fp32 device tensors in the reference layout.  layers: HOST array of n_dec_layers entries (egoego_layer_weights, with 256 in
 * place of 512).  head_w / head_b: the MLP heads' nn.Linear tensors in order —
 *   HeadNet:    action_va_mlp.affine_layers.0..2, action_va_fc, action_dist_mlp.affine_layers.0..2, action_dist_fc (8 entries);
 *   GravityNet: action_normal_mlp.affine_layers.0..1, action_normal_fc (3 entries, the rest NULL). */
typedef struct {
    const float* start_conv_w; const float* start_conv_b;  /* (256, d_feats, 1), (256) */
    const float* position_vec;                              /* (window + 1, 256) */
    const egoego_layer_weights* layers;
    const float* head_w[8];
    const float* head_b[8];
} egoego_s1_weights;

const char* egoego_s1_last_error(void);
int egoego_s1_ctx_create(const egoego_s1_config* cfg, int device, egoego_s1_ctx** out);
void egoego_s1_ctx_destroy(egoego_s1_ctx* ctx);
/* Packs the weights into split-bf16 fragment-tiled planes; synchronises `stream`. */
int egoego_s1_load_weights(egoego_s1_ctx* ctx, const egoego_s1_weights* w, void* stream);
/* Scratch bytes of a call over n_windows windows (0 if the shape is not accepted). */
size_t egoego_s1_workspace_bytes(const egoego_s1_ctx* ctx, int n_windows);

/* HE:123-170 / HN:118-155 for W windows in one launch per stage (embed, then per layer Q/K/V projection, attention, fused tail,
 * then the heads).  HeadNet: d_out [W][window][4] = (va xyz, distance scalar) of every token (padded tokens included);
 * GravityNet: d_out [W][3] = the floor normal from token 0.  d_layers (optional, NULL = none): the encoder output of every layer,
 * [n_dec_layers][W][window][256]. */
int egoego_s1_encode(egoego_s1_ctx* ctx, const float* d_feats, const int32_t* d_valid, int n_windows, float* d_out,
                     float* d_layers, void* d_workspace, size_t workspace_bytes, void* stream);

/* GravityNet's per-frame input (HN:118-145): d_rot [S][Lmax][3][3] and d_trans [S][Lmax][3] fp32 (the first len[s] frames of
 * each sequence), d_len int32 [S] -> d_feats [S][window][18] (frames truncated to window + 1, zero padded) and d_valid int32 [S]
 * = min(len, window + 1) - 1. */
int egoego_s1_gravity_features(const float* d_rot, const float* d_trans, const int32_t* d_len, int S, int Lmax, int window,
                               float* d_feats, int32_t* d_valid, void* stream);

/* HeadNet's integration and SLAM rescale (HE:97-119, 180-212, 214-308), fp64, one thread per sequence.  Sequence s has T[s]
 * frames in the consecutive windows win0[s].. of d_heads ([*][window][4], egoego_s1_encode's output); q0 [S][4] (w,x,y,z) is
 * its first head rotation; d_slam [S][Lmax][3] its aligned SLAM translation of len[s] frames.  Outputs: d_quat [S][Qmax][4]
 * (T[s] + 1 rotations, at most Qmax), d_trans [S][Lmax][3] (len[s] rescaled positions), d_scale [S] (pred_scale). */
int egoego_s1_integrate(const float* d_heads, int window, const int32_t* d_T, const int32_t* d_win0, const double* d_q0,
                        const double* d_slam, const int32_t* d_len, int S, int Lmax, int Qmax, float dist_scale,
                        double* d_quat, double* d_trans, double* d_scale, void* stream);

/* GravityNet's trajectory (HN:230-294 around the host's Rodrigues and Umeyama steps), fp64, one thread per sequence:
 * a_0 = 0, a_i = a_{i-1} + scale[s] Rn[s] (p_i - p_{i-1});  d_pose [S][Lmax][7] = (Ralign[s] a_i + origin[s], quat(Ralign[s] Rn[s] R_i))
 * with w >= 0.  d_rot / d_trans / d_len as for egoego_s1_gravity_features; Rn, Ralign [S][3][3], scale [S], origin [S][3]. */
int egoego_s1_gravity_apply(const float* d_rot, const float* d_trans, const int32_t* d_len, int S, int Lmax, const double* d_Rn,
                            const double* d_scale, const double* d_Ralign, const double* d_origin, double* d_pose, void* stream);

/* The two 3 x 3 steps between GravityNet's normal and egoego_s1_gravity_apply (HN:47-63 and evo's Umeyama alignment, HN:230-270),
 * fp64, one workgroup per sequence; no context, no workspace.  d_rot is not read (the alignment sees positions only) and may be
 * NULL; d_trans / d_len as for egoego_s1_gravity_apply; d_normal [S][3] fp32 (egoego_s1_encode's GravityNet output); d_scale [S];
 * d_ref [S][Rmax][7] fp64 (xyz + quaternion, only xy is read) with d_ref_len int32 [S].
 *   d_Rn [S][3][3]      the Rodrigues rotation taking the normal onto +z, rounded through fp32 (a normal parallel to z divides by
 *                       zero, as the reference's formula does)
 *   d_Ralign [S][3][3]  evo's Umeyama rotation of est_i = p_0 + sum_{k<=i} scale Rn (p_k - p_{k-1}) onto ref_i over the first
 *                       n = min(len, ref_len) frames with z set to 1, rounded through fp32: blockdiag(Q, det Q), Q the orthogonal
 *                       polar factor of the 2 x 2 covariance (closed form, no SVD).  Identity when the covariance is zero (n <= 1).
 *                       On a straight line (rank-1 covariance) the reference's own answer is arbitrary between the rotation and the
 *                       z-flipping reflection; the result is then only promised finite, orthonormal, det +1.
 * The frames are summed in a fixed order (serial chain, per-lane fp64 partials folded in lane order): a sequence's result does not
 * depend on the batch around it or on Lmax / Rmax. */
int egoego_s1_gravity_align(const float* d_rot, const float* d_trans, const int32_t* d_len, int S, int Lmax, const float* d_normal,
                            const double* d_scale, const double* d_ref, const int32_t* d_ref_len, int Rmax, double* d_Rn,
                            double* d_Ralign, void* stream);

/* egoego/eval/head_pose_metrics.py compute_head_pose_metrics for B sequences, fp64, one workgroup per sequence; no context, no
 * workspace.  d_pred / d_gt [B][Tmax][7] fp64 (xyz + quaternion w,x,y,z, converted by pytorch3d's quaternion_to_matrix formula),
 * d_lengths int32 [B] (1..Tmax; frames past it are never read) -> d_out [B][3] = (head_dist, head_dist_rot_only, head_trans_err
 * in mm), each a per-frame sum in a fixed order divided by the length.  With E = Rp Rg^-1 (3 x 3 inverse by adjugate):
 * head_dist = sqrt(|I - E|_F^2 + |tp - E tg|^2) (= |I4 - X Y^-1|_F), head_dist_rot_only = |I3 - E|_F, head_trans_err = |tp - tg|. */
int egoego_s1_head_pose_metrics(const double* d_pred, const double* d_gt, const int32_t* d_lengths, int B, int Tmax, double* d_out,
                                void* stream);

/* ==================================================================================================================
 * Stage 1's optical-flow feature extractor: FeatureExtractor (egoego/model/resnet.py = RN, lines 25-50), i.e. torchvision's
 * resnet18 with fc = Linear(512, 512), in eval mode (BatchNorm with its running statistics, eps 1e-5), on 224 x 224 flow
 * fields.  Every convolution and the fc run as split-bf16 implicit GEMMs (three bf16 MFMAs, fp32 accumulate) over fp32 NHWC
 * activations.  Frames run in chunks of at most `chunk_frames` through a caller-allocated workspace; a frame's features are
 * bit-identical whatever the chunk, the position or the other frames of the call.  egoego_flow_last_error() describes the last
 * failure of an egoego_flow_* call.
 * ================================================================================================================== */
typedef struct egoego_flow_ctx egoego_flow_ctx;

/* fp32 device tensors in the reference layout (the state dict of RN ResNet.resnet).  The 20 convolutions and their BatchNorms
 * in this order: conv1 / bn1; then for layer1..layer4, block 0..1: conv1 / bn1, conv2 / bn2, and for block 0 of layer2..4
 * downsample.0 / downsample.1 — i.e. index 0 stem, 1-4 layer1, 5-9 layer2, 10-14 layer3, 15-19 layer4.  conv_w[0] is
 * (64, 3, 7, 7); its third input channel multiplies the reference's all-zero third flow channel and is not read. */
typedef struct {
    const float* conv_w[20];   /* (Cout, Cin, kh, kw) */
    const float* bn_w[20];     /* (Cout) */
    const float* bn_b[20];
    const float* bn_mean[20];  /* running_mean */
    const float* bn_var[20];   /* running_var */
    const float* fc_w;         /* (512, 512) */
    const float* fc_b;         /* (512) */
} egoego_flow_weights;

const char* egoego_flow_last_error(void);
/* chunk_frames: frames per pass through the workspace (0 = the default, 256). */
int egoego_flow_ctx_create(int device, int chunk_frames, egoego_flow_ctx** out);
void egoego_flow_ctx_destroy(egoego_flow_ctx* ctx);
/* RN:5-23 (ResNet.__init__): packs the convolution weights as [Cout][kh][kw][Cin] split-bf16 fragment-tiled planes and folds
 * every BatchNorm into a per-channel fp32 scale = w / sqrt(var + 1e-5) and shift = b - mean * scale; synchronises `stream`. */
int egoego_flow_load_weights(egoego_flow_ctx* ctx, const egoego_flow_weights* w, void* stream);
/* Scratch bytes of a call over n_frames frames: min(n_frames, chunk_frames) frames' activations (0 if not accepted). */
size_t egoego_flow_workspace_bytes(const egoego_flow_ctx* ctx, int n_frames);
/* RN:38-50 (FeatureExtractor.forward) for N frames: d_flow [N][224][224][2] fp32 (the flow's two channels; the reference's
 * appended zero channel is implied) -> d_out [N][512] fp32.  23 launches per chunk.  d_stages (optional, NULL = none): the
 * activations after the stem (conv1, bn1, ReLU, max-pool) and after each of layer1..4, NHWC fp32, one array after the other:
 * [N][56][56][64], [N][56][56][64], [N][28][28][128], [N][14][14][256], [N][7][7][512]. */
int egoego_flow_features(egoego_flow_ctx* ctx, const float* d_flow, int n_frames, float* d_out, float* d_stages,
                         void* d_workspace, size_t workspace_bytes, void* stream);

/* ==================================================================================================================
 * The SMPL-H body model: what run_smpl_model (egoego/data/amass_diffusion_dataset.py = AD, lines 15-81) reaches through
 * human_body_prior's BodyModel — shape blend, Rodrigues, pose-corrective blend shapes, the kinematic chain and linear-blend
 * skinning, 52 joints, any vertex count.  The pose blend shapes run as one split-bf16 GEMM (three bf16 MFMAs, fp32 accumulate)
 * with the skinning fused into its epilogue; the per-frame geometry is fp64, one thread per frame.  Frames run in chunks of at
 * most `chunk_frames` through a caller-allocated workspace; a frame's vertices are bit-identical whatever the chunk, the
 * position or the other frames of the call.  egoego_body_last_error() describes the last failure of an egoego_body_* call.
 * ================================================================================================================== */
typedef struct egoego_body_ctx egoego_body_ctx;

/* Device tensors.  j_template = J_regressor . v_template and j_shapedirs = J_regressor . shapedirs are computed by the caller
 * (fp64, rounded once); the skinning weights come compressed to n_weights (joint, weight) pairs per vertex, pair k of vertex v
 * at [k][v], padded with (0, 0.0f). */
typedef struct {
    int32_t n_verts;
    int32_t n_betas;
    int32_t n_weights;           /* 1..52 */
    const float* v_template;     /* (V, 3) */
    const float* shapedirs;      /* (V, 3, n_betas) */
    const float* posedirs;       /* (V, 3, 459), k = 9 (joint - 1) + 3 row + col of R - I */
    const float* j_template;     /* (52, 3) */
    const float* j_shapedirs;    /* (52, 3, n_betas) */
    const float* skin_weight;    /* (n_weights, V) */
    const int32_t* skin_joint;   /* (n_weights, V) */
    const int32_t* parents;      /* (52): kintree_table[0]; parents[j] < j for j >= 1, parents[0] is not read */
} egoego_body_model;

const char* egoego_body_last_error(void);
/* chunk_frames: frames per pass through the workspace (0 = the default, 8192). */
int egoego_body_ctx_create(int device, int chunk_frames, egoego_body_ctx** out);
void egoego_body_ctx_destroy(egoego_body_ctx* ctx);
/* Copies the model and packs posedirs into split-bf16 fragment-tiled planes (rows ordered so that the x, y and z of a vertex
 * fall to one lane, K padded to 480); synchronises `stream`. */
int egoego_body_load_model(egoego_body_ctx* ctx, const egoego_body_model* m, void* stream);
/* Scratch bytes of a call over n_frames frames of n_seqs sequences (0 if not accepted or no model is loaded). */
size_t egoego_body_workspace_bytes(const egoego_body_ctx* ctx, int n_frames, int n_seqs);
/* N frames: d_root_orient [N][3], d_pose_body [N][63], d_pose_hand [N][90] (NULL = identity hand rotations: K runs over the 21
 * body joints only, bit-identical to a zero hand pose), d_trans [N][3], axis-angle fp32; d_betas [n_seqs][n_betas] and
 * d_seq int32 [N], each frame's row of d_betas -> d_verts [N][V][3], d_joints [N][52][3] fp32.  d_pose_offsets (optional,
 * NULL = none): [N][V][3], the pose-corrective offsets posedirs . (R - I) alone.  Two launches per call and two per chunk. */
int egoego_body_forward(egoego_body_ctx* ctx, const float* d_root_orient, const float* d_pose_body, const float* d_pose_hand,
                        const float* d_trans, const float* d_betas, const int32_t* d_seq, int n_frames, int n_seqs,
                        float* d_verts, float* d_joints, float* d_pose_offsets, void* d_workspace, size_t workspace_bytes,
                        void* stream);

/* ==================================================================================================================
 * Batched evaluation of sampled motions: what the reference's evaluation loop (eval_egoego.py:358-446) does per sample on the
 * host — fk_smpl, determine_floor_height_and_contacts (utils/data_utils/process_amass_dataset.py:160-338, with sklearn's
 * DBSCAN restated on the sorted line) and compute_metrics_for_smpl (kinpoly/scripts/eval_metrics_imu_rec.py:264-342) — for B
 * sequences of 22 joints at once.  Every tensor is a device tensor; sequences are padded to T frames and d_lengths (int32 [B],
 * NULL = all T) gives each one's real length; padded frames are never read into a result.  The entries keep no state.  A
 * sequence's results are bit-identical alone, at any position of a batch and under any padded T.
 * egoego_eval_last_error() describes the last failure of an egoego_eval_* call.
 * ================================================================================================================== */
const char* egoego_eval_last_error(void);
/* The longest sequence egoego_eval_floor_contacts accepts (4096): 2 T static-height samples are kept in LDS. */
int egoego_eval_max_frames(void);
/* fk_smpl for N frames: d_root [N][3], d_aa [N][22][3] local axis-angle, d_rest_offsets [22][3]; parents_host: 22 ints on the
 * host, parents[j] < j for j >= 1 -> d_quat [N][22][4] global rotations (w, x, y, z; w >= 0), d_jpos [N][22][3].  fp64 inside,
 * rounded once. */
int egoego_eval_fk(const float* d_root, const float* d_aa, const float* d_rest_offsets, const int32_t* parents_host, int n_frames,
                   float* d_quat, float* d_jpos, void* stream);
/* d_jpos [B][T][22][3], in place: every joint of sequence b moves by minus the xy of `joint` in its first frame. */
int egoego_eval_shift_xy(float* d_jpos, int B, int T, int joint, void* stream);
/* determine_floor_height_and_contacts for B sequences d_jpos [B][T][22][3] (z up), T <= egoego_eval_max_frames():
 * d_floor_height, d_offset_floor_height (= floor - 0.01; both 0 without a static toe sample) [B] fp32; d_contacts [B][T][22]
 * fp32 0 / 1 (zero on padded frames); d_discard [B] int32; d_n_static [B]: the number of static toe samples n; d_n_groups [B]:
 * clusters plus the noise group if any.  d_labels (optional, NULL = none): int32 [B][2 T], the DBSCAN label of each sample in
 * the reference's order (left-toe frames, then right-toe frames), -1 = noise, -2 past n.  One workgroup per sequence. */
int egoego_eval_floor_contacts(const float* d_jpos, const int32_t* d_lengths, int B, int T, float fps, float* d_floor_height,
                               float* d_offset_floor_height, float* d_contacts, int32_t* d_discard, int32_t* d_labels,
                               int32_t* d_n_static, int32_t* d_n_groups, void* stream);
/* compute_metrics_for_smpl for B predictions d_pred_quat [B][T][22][4], d_pred_jpos [B][T][22][3] against the ground truth
 * d_gt_quat / d_gt_jpos ([T]... shared by all when gt_shared != 0, else [B][T]...); floor heights [B] fp32 each.
 * d_out [B][35] fp64: root_dist, root_rot_dist, root_trans_dist, head_dist, head_rot_dist, head_trans_dist, mpjpe,
 * mpjpe_wo_hand, accel_pred, accel_gt, accel_err, pred_fs, gt_fs, then single_jpe[22]; the reference's units.  The
 * acceleration terms need 3 frames (NaN below).  One workgroup per prediction; fp64 sums in a fixed order. */
int egoego_eval_metrics(const float* d_gt_quat, const float* d_gt_jpos, int gt_shared, const float* d_gt_floor_height,
                        const float* d_pred_quat, const float* d_pred_jpos, const float* d_pred_floor_height,
                        const int32_t* d_lengths, int B, int T, double* d_out, void* stream);
/* d_root [B][T][3] = joint 0 of d_jpos [B][T][22][3] with d_floor_height[b] taken off z. */
int egoego_eval_root_to_floor(const float* d_jpos, const float* d_floor_height, int B, int T, float* d_root, void* stream);
/* d_best [n_groups] int32: per group g the first b with d_group[b] == g (NULL = all 0) whose d_metrics[b][column] is smallest,
 * -1 for an empty group. */
int egoego_eval_best(const double* d_metrics, int column, const int32_t* d_group, int B, int n_groups, int32_t* d_best, void* stream);

/* ==================================================================================================================
 * Stage-2 motion windows (egoego_win_*; added under ABI 8, purely additive): raw SMPL-H motion -> what the reference's
 * AMASSDataset stores per window (egoego/data/amass_diffusion_dataset.py:409-510), its min / max statistics (355-377) and the
 * normalised model input of __getitem__ (515-538).  Every tensor is a device tensor unless it says host.  The frames of all
 * sequences are concatenated ([F] rows); window n covers the d_length[n] (0..W) frames from row d_first[n] and is padded with
 * zero rows to W.  A window whose rows would leave the [F] frames is written as an empty one.  The entries keep no state.  A
 * window's rows depend on its own frames only: they are bit-identical alone, anywhere in a batch and under any W that holds them.
 * egoego_win_last_error() describes the last failure of an egoego_win_* call.
 * ================================================================================================================== */
const char* egoego_win_last_error(void);
/* The largest window W the entries accept: a window's positions stay in LDS. */
int egoego_win_max_window(void);
/* d_trans [F][3], d_root_orient [F][3], d_body_pose [F][63], d_rest_offsets [22][3]; parents_host: 22 ints on the host,
 * parents[j] < j for j >= 1.  Per window: d_jpos [N][W][66] (joints after FK, turned by the inverse of the first frame's head
 * heading when `canonicalize` is set, shifted so that this head's xy is 0), d_jvel [N][W][66] (jpos[t + 1] - jpos[t] on the fp32
 * values; zero in the last real frame), d_grot6d / d_lrot6d [N][W][132] (the first two rows of the global / local rotation
 * matrices), d_recover [N][4] (the heading quaternion w, x, y, z; the identity without `canonicalize`).  fp64 inside, each output
 * rounded once.  One workgroup per window. */
int egoego_win_build(const float* d_trans, const float* d_root_orient, const float* d_body_pose, int n_frames, const float* d_rest_offsets,
                     const int32_t* parents_host, const int32_t* d_first, const int32_t* d_length, int N, int W, int canonicalize,
                     float* d_jpos, float* d_jvel, float* d_grot6d, float* d_lrot6d, float* d_recover, void* stream);
/* d_stats [4][66]: min jpos, max jpos, min jvel, max jvel per coordinate over the real frames of all N windows (the zero
 * velocity of each window's last frame included), exactly.  The workspace (256-byte aligned) holds the per-workgroup partials. */
size_t egoego_win_stats_workspace_bytes(int N, int W);
int egoego_win_stats(const float* d_jpos, const float* d_jvel, const int32_t* d_length, int N, int W, float* d_stats, void* workspace,
                     size_t workspace_bytes, void* stream);
/* d_motion [N][W][198]: (jpos - min) / (max - min) * 2 - 1 in fp32 (d_jpos_min / d_jpos_max [66]; a coordinate with max == min
 * divides by zero, as in the reference), then d_grot6d; zero rows past each length. */
int egoego_win_motion(const float* d_jpos, const float* d_grot6d, const int32_t* d_length, const float* d_jpos_min, const float* d_jpos_max,
                      int N, int W, float* d_motion, void* stream);

/* ==================================================================================================================
 * AMASS preprocessing (egoego_amass_*; added under ABI 8, purely additive): raw AMASS sequences -> the records of the reference's
 * process_seq (utils/data_utils/process_amass_dataset.py:340-493).  Every tensor is a device tensor unless it says host.  The raw
 * frames of all B sequences are packed end to end ([N] rows): sequence b owns rows offsets[b] .. offsets[b + 1], offsets[0] = 0,
 * offsets[B] = N.  Memory grows with N, never with B times the longest sequence.  The entries keep no state.  A sequence's
 * results depend on its own frames only: they are bit-identical alone, anywhere in a batch and next to any neighbours.
 * egoego_amass_last_error() describes the last failure of an egoego_amass_* call.
 * ================================================================================================================== */
const char* egoego_amass_last_error(void);
/* The longest sequence egoego_amass_floor_contacts accepts (65536 raw frames). */
int egoego_amass_max_frames(void);
/* The first 22 joints of the body model at zero betas for N frames: d_root_orient [N][3], d_pose_body [N][63], d_trans [N][3]
 * (the poses already rounded to fp32), d_j_template [22][3] (the model's rest joints); parents_host: 22 ints on the host,
 * parents[j] < j for j >= 1 -> d_joints [N][22][3] (chain + trans) and d_head_rot [N][9], the global rotation of joint 15,
 * row-major.  fp64 inside, rounded once. */
int egoego_amass_joints(const float* d_root_orient, const float* d_pose_body, const float* d_trans, const float* d_j_template,
                        const int32_t* parents_host, int n_frames, float* d_joints, float* d_head_rot, void* stream);
/* Bytes of workspace egoego_amass_floor_contacts needs for B sequences of n_frames frames in all (0 = bad shape). */
size_t egoego_amass_floor_workspace_bytes(int n_frames, int B);
/* determine_floor_height_and_contacts (:160-338) for B packed sequences d_joints [N][22][3] (z up) at their own frame rates:
 * d_size_thresh [B] int32 holds int(0.25 * fps) per sequence.  offsets_host: B + 1 ints on the host, validated (every sequence
 * 1..egoego_amass_max_frames() frames); d_offsets: the same values on the device.  Outputs as egoego_eval_floor_contacts, packed:
 * d_floor_height, d_offset_floor_height, d_discard, d_n_static, d_n_groups [B]; d_contacts [N][22]; d_labels (optional) int32
 * [2 N], sequence b's 2 L entries from 2 * offsets[b].  A sequence of at most egoego_eval_max_frames() frames runs in LDS, a
 * longer one (and every one when force_long != 0) in its slice of the workspace, with the same arithmetic and the same bits.
 * The workspace (256-byte aligned) may hold any bytes on entry.  One workgroup per sequence. */
int egoego_amass_floor_contacts(const float* d_joints, const int32_t* offsets_host, const int32_t* d_offsets, const int32_t* d_size_thresh,
                                int B, int force_long, float* d_floor_height, float* d_offset_floor_height, float* d_contacts,
                                int32_t* d_discard, int32_t* d_labels, int32_t* d_n_static, int32_t* d_n_groups, void* workspace,
                                size_t workspace_bytes, void* stream);
/* The saved tracks (:443-472) for n_out output frames: output frame i of sequence d_seq[i] is raw frame d_src[i] (the downsample
 * table plus the sequence's first row); d_out_offsets [B + 1] delimits each sequence's output frames.  d_joints_out [n_out][22][3]
 * (z minus d_offset_floor_height[b]), d_contacts_out [n_out][22] fp64, d_head_trans [n_out][3], d_rot6d [n_out][6], d_qpos
 * [n_out][7] (position, then w, x, y, z with w >= 0), d_rot6d_diff [n_out][6] and d_trans_diff [n_out][3] (frame t + 1 against t;
 * zero in a sequence's last row), d_vels [n_out][6] (get_head_vel :111-137; the last row repeats the one before), d_same [n_out]
 * uint8: 1 where the pair took the |1 -+ q0| < 1e-6 branch.  fp64 from the fp32 inputs, rounded once. */
int egoego_amass_head(const float* d_joints, const float* d_head_rot, const float* d_contacts, const float* d_offset_floor_height,
                      const int32_t* d_src, const int32_t* d_seq, const int32_t* d_out_offsets, int n_out, int n_frames, int B,
                      float* d_joints_out, double* d_contacts_out, float* d_head_trans, float* d_rot6d, float* d_qpos, float* d_rot6d_diff,
                      float* d_trans_diff, float* d_vels, uint8_t* d_same, void* stream);

/* ==================================================================================================================
 * The stage-2 training step (egoego_train_*; added under ABI 8, purely additive): the loss of CondGaussianDiffusion.p_losses
 * (M:574-605) and the gradient of every trainable tensor of the denoiser, on split-bf16 MFMAs (three bf16 MFMAs per product, fp32
 * accumulate; LayerNorm, softmax, GELU, residuals and the loss in fp32, the loss summed in fp64 in a fixed order).  Shapes:
 * d_model 512, 4 heads, d_k = d_v = 256, FFN 512; n_dec_layers and d_feats from the config; T + 1 <= 197.
 *   - the weights are the caller's LIVE fp32 parameter tensors (egoego_weights, device pointers): every call reads them in place
 *     and splits them as it loads them, so a call after an optimizer step sees the new values; nothing is packed or cached.
 *   - a call only enqueues work on `stream`: no allocation, no host copy, no synchronisation.
 *   - `saves` is a caller-allocated buffer (256-byte aligned, egoego_train_saves_bytes) that egoego_train_forward fills and
 *     egoego_train_backward reads: one per outstanding graph.  The workspace (egoego_train_workspace_bytes) is scratch of one call;
 *     what either buffer holds on entry to egoego_train_forward is irrelevant, as for every other workspace of this library.
 *   - every sum over the B * (T + 1) rows (weight, bias and LayerNorm gradients) runs over fixed chunks of rows whose partials are
 *     added in chunk order, without float atomics: loss and gradients have the same bits on every run.
 *   - dropout (TM:63, 68, 108: attention probabilities, fc output, FFN output) draws in-kernel Philox4x32-10 keyed by
 *     (seed; layer, site, window id, element index within the window); the backward pass regenerates the masks.  p_drop = 0: none.
 * egoego_train_last_error() describes the last failure of an egoego_train_* call.
 * ================================================================================================================== */
typedef struct egoego_train_ctx egoego_train_ctx;
enum { EGOEGO_LOSS_L1 = 0, EGOEGO_LOSS_L2 = 1 };  /* M:563-571 */
enum { EGOEGO_TRAIN_SITE_ATTN = 0, EGOEGO_TRAIN_SITE_FC = 1, EGOEGO_TRAIN_SITE_FFN = 2 };
/* egoego_train_saved: [B][T+1][512] unless noted */
enum { EGOEGO_TRAIN_SAVED_FFN_HIDDEN = 0,  /* relu(w_1 . + b_1) */
       EGOEGO_TRAIN_SAVED_ATTN_PROB = 1,   /* [B][4][T+1][T+1], before dropout */
       EGOEGO_TRAIN_SAVED_ATTN_OUT = 2,    /* [B][T+1][1024] */
       EGOEGO_TRAIN_SAVED_ATTN_LN = 3,     /* the attention sublayer's output */
       EGOEGO_TRAIN_SAVED_LAYER_OUT = 4,
       EGOEGO_TRAIN_SAVED_LAYER_IN = 5 };

/* Caller-allocated fp32 device buffers, one per trainable tensor, in the layout of egoego_weights (conv weights (out, in, 1)).
 * position_vec is frozen: its slot is not read. */
typedef struct {
    float* w_q; float* b_q; float* w_k; float* b_k; float* w_v; float* b_v; float* w_fc; float* b_fc; float* ln1_g; float* ln1_b;
    float* w_1; float* b_1; float* w_2; float* b_2; float* ln2_g; float* ln2_b;
} egoego_train_layer_grads;
typedef struct {
    float* start_conv_w; float* start_conv_b;
    float* position_vec;  /* unused */
    float* linear_out_w; float* linear_out_b;
    float* time_mlp1_w; float* time_mlp1_b;
    float* time_mlp3_w; float* time_mlp3_b;
    const egoego_train_layer_grads* layers;  /* HOST array of n_dec_layers entries */
} egoego_train_grads;

const char* egoego_train_last_error(void);
/* cfg: the shapes of egoego_config (objective, precision and flags are not read). */
int egoego_train_ctx_create(const egoego_config* cfg, int device, egoego_train_ctx** out);
void egoego_train_ctx_destroy(egoego_train_ctx* ctx);
/* 0 (egoego_train_last_error() says why) for a shape no call accepts. */
size_t egoego_train_workspace_bytes(const egoego_train_ctx* ctx, int B, int T);
size_t egoego_train_saves_bytes(const egoego_train_ctx* ctx, int B, int T);
/* p_losses (M:574-605) with the caller's draws: d_x_start, d_noise, d_cond_noise, d_cond_mask [B][T][d_feats]; d_t int64 [B]
 * (clamped to the schedule); d_row_mask fp32 [B][T+1] (padding_mask[:, 0, :]) or NULL; the three schedule tables are DEVICE arrays
 * of num_timesteps entries (sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod, p2_loss_weight).  d_window_ids int64 [B] or NULL
 * (window b has id b): the dropout streams.  Writes *d_loss (device scalar) and, when not NULL, d_model_out [B][T][d_feats].
 * The rows of d_model_out of a window depend on that window's own inputs and id only. */
int egoego_train_forward(egoego_train_ctx* ctx, const egoego_weights* w, const float* d_x_start, const float* d_noise,
                         const float* d_cond_noise, const float* d_cond_mask, const int64_t* d_t, const float* d_row_mask,
                         const float* d_sqrt_alphas_cumprod, const float* d_sqrt_one_minus_alphas_cumprod, const float* d_p2_loss_weight,
                         int objective, int loss_type, float p_drop, uint64_t dropout_seed, const int64_t* d_window_ids, int B, int T,
                         void* d_saves, size_t saves_bytes, void* d_workspace, size_t workspace_bytes, float* d_loss, float* d_model_out,
                         void* stream);
/* The gradient of d_upstream[0] * loss for every buffer of `grads` (overwritten), from the saves of the forward call with the same
 * weights, p_drop, dropout_seed, B and T.  d_upstream is a DEVICE scalar: the product is taken on the device, and a power of two
 * scales every gradient exactly. */
int egoego_train_backward(egoego_train_ctx* ctx, const egoego_weights* w, const void* d_saves, size_t saves_bytes,
                          const float* d_upstream, const egoego_train_grads* grads, float p_drop, uint64_t dropout_seed, int B, int T,
                          void* d_workspace, size_t workspace_bytes, void* stream);
/* The mask (1 keep / 0 drop, one byte each) a forward call with these arguments applies at `site` of `layer`: site 0
 * [B][4][T+1][T+1], sites 1 and 2 [B][T+1][512].  The workspace holds the implied window ids when d_window_ids is NULL (8 B bytes). */
int egoego_train_dropout_mask(egoego_train_ctx* ctx, float p_drop, uint64_t dropout_seed, int layer, int site, const int64_t* d_window_ids,
                              int B, int T, uint8_t* d_out, void* d_workspace, size_t workspace_bytes, void* stream);
/* Test/debug: copies saved tensor `which` (EGOEGO_TRAIN_SAVED_*) of `layer` out of the saves of a forward call. */
int egoego_train_saved(egoego_train_ctx* ctx, const void* d_saves, size_t saves_bytes, int B, int T, int layer, int which, float* d_out,
                       void* stream);

/* ==================================================================================================================
 * The fused parameter update (egoego_optim_*; added under ABI 8, purely additive): gradient norm, NaN skip, unscale, Adam
 * (torch.optim.Adam, amsgrad off), ema-pytorch's EMA and gradient clearing over a list of fp32 contiguous device tensors, each with
 * a gradient, exp_avg and exp_avg_sq of its own size and, optionally, an EMA tensor.  One step is three launches on `stream`:
 * one partial sum of (g * inv_scale)^2 per chunk of EGOEGO_OPTIM_CHUNK elements (fp64, fixed order); one workgroup that adds the
 * partials in a fixed order (thread t the partials of its run of consecutive chunks in chunk order, then the 256 sums in thread
 * order), decides whether the step is skipped, advances the counters and writes this step's scalars, all in fp64 rounded once;
 * and the update itself.  Nothing is read back: a skipped step (NaN norm, NaN loss, found_inf) writes no parameter, moment or EMA
 * value, and the step counters stay.
 *   - the caller allocates everything: the moments, the state block (egoego_optim_state_bytes, 256-byte aligned, zeroed before
 *     the first use) and the workspace (egoego_optim_workspace_bytes).  The state block begins with an egoego_optim_state and
 *     holds the descriptor tables (tensor -> pointers, chunk -> tensor, offset, count) behind it; together with the EMA's two
 *     counters (device scalars of the caller, as ema-pytorch keeps them) it is the only memory that carries meaning from call to
 *     call.  What the workspace holds on entry is irrelevant.
 *   - a call only enqueues work on `stream`: no allocation, no copy through the host, no synchronisation, no float atomics.
 *   - a tensor may start at any 4-byte offset: 16-byte accesses are used where all tensors of an entry share their 16-byte phase.
 * egoego_optim_last_error() describes the last failure of an egoego_optim_* call.
 * ================================================================================================================== */
typedef struct egoego_optim_ctx egoego_optim_ctx;
#define EGOEGO_OPTIM_CHUNK 4096
#define EGOEGO_OPTIM_MAX_LOSSES 8
enum { EGOEGO_OPTIM_SKIP_NAN = 0,         /* the reference's rule (trainer:144-160): NaN only */
       EGOEGO_OPTIM_SKIP_NONFINITE = 1 }; /* +-inf as well */
enum { EGOEGO_OPTIM_EMA_NONE = 0, EGOEGO_OPTIM_EMA_COPY = 1, EGOEGO_OPTIM_EMA_LERP = 2 };

/* The head of the state block.  Counters first, then what the last call decided. */
typedef struct {
    int64_t adam_step;      /* applied Adam steps: the `step` of torch.optim.Adam's state */
    int64_t applied;        /* calls that were not skipped */
    int64_t skipped;        /* calls that were */
    double total_norm;      /* sqrt(sum (g * inv_scale)^2) of the last call with do_adam */
    float total_norm_f32;
    int32_t last_skip;      /* 1: the last call was skipped */
    float step_size;        /* lr / (1 - beta1^step) */
    float bc2_sqrt;         /* sqrt(1 - beta2^step) */
    float one_minus_decay;  /* of the last lerp */
    int32_t ema_action;     /* EGOEGO_OPTIM_EMA_* of the last call */
    float clip_coef;        /* min(1, max_norm / (total_norm + clip_eps)) of the last call; 1 without clipping or when skipped */
} egoego_optim_state;

typedef struct {
    double lr, beta1, beta2, eps, weight_decay;  /* weight_decay: torch's L2 form, g + weight_decay * p */
} egoego_optim_hyper;

/* egoego_optimw_step's hyper-parameters: the five above, then
 *   decoupled  0: weight_decay is the L2 term.  1: torch.optim.AdamW's form, p *= (float)(1 - lr * weight_decay) (the factor
 *              formed in double, rounded once) before an Adam step without the L2 term;
 *   max_norm   > 0: torch.nn.utils.clip_grad_norm_ inside the step.  decide computes coef = min(1, max_norm / (total_norm +
 *              clip_eps)) in fp64 from the fp64 norm and rounds it once to egoego_optim_state.clip_coef; the update uses
 *              (g * inv_scale) * clip_coef, two fp32 products in torch's order.  The gradients in memory are NOT rewritten
 *              with their clipped values (torch clips in place): they keep their bits, or are cleared by zero_grads.
 *              <= 0: no clipping; NaN is refused;
 *   clip_eps   clip_grad_norm_'s 1e-6; >= 0. */
typedef struct {
    double lr, beta1, beta2, eps, weight_decay;
    int decoupled;
    double max_norm, clip_eps;
} egoego_optim_hyper_w;

/* ema-pytorch's schedule: a call with do_ema reads *d_step, adds one, and acts only when the value it read is a multiple of
 * update_every: a copy up to update_after_step and, once, on the first call after it (which sets *d_initted = 1); afterwards
 * ema -= (ema - p) * (1 - decay), decay = clamp(1 - (1 + e / inv_gamma)^-power, min_value, beta), e = step read - update_after_step. */
typedef struct {
    double beta, inv_gamma, power, min_value;
    int64_t update_every, update_after_step;
    int64_t* d_step;   /* device scalar */
    float* d_initted;  /* device scalar: 0 or 1 */
} egoego_optim_ema;

const char* egoego_optim_last_error(void);
/* counts: HOST array of n_tensors element counts (each >= 1). */
int egoego_optim_ctx_create(int device, int n_tensors, const int64_t* counts, egoego_optim_ctx** out);
void egoego_optim_ctx_destroy(egoego_optim_ctx* ctx);
size_t egoego_optim_workspace_bytes(const egoego_optim_ctx* ctx);
size_t egoego_optim_state_bytes(const egoego_optim_ctx* ctx);
/* Writes the descriptor tables of d_state from HOST arrays of n_tensors device pointers each: the parameters; gradients, exp_avg
 * and exp_avg_sq (all three NULL for a context that only ever runs do_adam = 0); the EMA tensors or NULL.  Call it once, and again
 * whenever one of the pointers has changed.  The counters of d_state are not touched. */
int egoego_optim_set_tensors(egoego_optim_ctx* ctx, float* const* p, float* const* g, float* const* m, float* const* v, float* const* ema,
                             void* d_state, size_t state_bytes, void* stream);
/* One step.  losses: HOST array of n_losses (<= 8) pointers to device scalars, or NULL; d_inv_scale, d_found_inf: device scalars
 * or NULL; do_adam = 0 runs the EMA alone (no norm, no moments); do_ema needs the EMA pointers of egoego_optim_set_tensors and
 * ema->d_step / d_initted; zero_grads needs do_adam and clears the gradients whether the step is skipped or not. */
int egoego_optim_step(egoego_optim_ctx* ctx, const egoego_optim_hyper* hyper, const egoego_optim_ema* ema, const float* const* losses,
                      int n_losses, const float* d_inv_scale, const float* d_found_inf, int skip_on, int zero_grads, int do_adam, int do_ema,
                      void* d_state, size_t state_bytes, void* d_workspace, size_t workspace_bytes, void* stream);
/* egoego_optim_step with decoupled weight decay and gradient clipping (egoego_optim_hyper_w); the same three launches, and
 * nothing else differs.  egoego_optim_step is this call with decoupled = 0, max_norm = 0.  A bad decoupled, a NaN max_norm or a
 * negative clip_eps is refused before any launch. */
int egoego_optimw_step(egoego_optim_ctx* ctx, const egoego_optim_hyper_w* hyper, const egoego_optim_ema* ema, const float* const* losses,
                        int n_losses, const float* d_inv_scale, const float* d_found_inf, int skip_on, int zero_grads, int do_adam, int do_ema,
                        void* d_state, size_t state_bytes, void* d_workspace, size_t workspace_bytes, void* stream);
/* Copies the egoego_optim_state at the head of d_state to d_out (device memory) on `stream`: the one call a caller may follow with
 * a synchronisation, to read counters for tests and logging. */
int egoego_optim_read_state(egoego_optim_ctx* ctx, const void* d_state, size_t state_bytes, egoego_optim_state* d_out, void* stream);

/* ==================================================================================================================
 * Stage-1 training (egoego_s1_train_*, egoego_s1_headnet_loss; added under ABI 8, purely additive): the training encode of
 * HeadNet and GravityNet (the TM Decoder at d_model 256 plus the ReLU MLP heads) with the gradient of every trainable tensor, and
 * HeadNet's loss (HE:97-119, 310-345) with its gradient with respect to the heads.  The conventions of egoego_train_* hold: the
 * weights are the caller's LIVE fp32 tensors (egoego_s1_weights, read in place, never packed); a call only enqueues work on
 * `stream` (no allocation, no host copy, no synchronisation); `saves` (256-byte aligned, egoego_s1_train_saves_bytes) is filled by
 * the forward call and read by the backward call, one per outstanding graph; the workspace is scratch of one call and neither
 * buffer's content on entry matters; every sum over rows runs over fixed chunks whose partials are added in order in fp64, without
 * float atomics; dropout (three sites per layer) is Philox keyed by (seed; layer, site, window id, element within the window).
 * Contractions are split-bf16 (three bf16 MFMAs, fp32 accumulate); LayerNorm, softmax and residuals fp32; the loss fp64.
 * egoego_s1_train_last_error() describes the last failure of any call of this section.
 * ================================================================================================================== */
typedef struct egoego_s1_train_ctx egoego_s1_train_ctx;
/* egoego_s1_train_saved: the EGOEGO_TRAIN_SAVED_* tensors of a decoder layer ([W][window][256], ATTN_PROB [W][4][window][window],
 * ATTN_OUT [W][window][1024]) and the heads' hidden rows (after the ReLU; `layer` then counts the heads' Linears as head_w does). */
enum { EGOEGO_S1_TRAIN_SAVED_HEAD_HIDDEN = 6 };

/* Caller-allocated fp32 device buffers, one per trainable tensor, in the layout of egoego_s1_weights.  position_vec is frozen:
 * its slot is not read. */
typedef struct {
    float* start_conv_w; float* start_conv_b;
    float* position_vec;  /* unused */
    const egoego_train_layer_grads* layers;  /* HOST array of n_dec_layers entries */
    float* head_w[8];
    float* head_b[8];
} egoego_s1_train_grads;

const char* egoego_s1_train_last_error(void);
/* cfg as for egoego_s1_ctx_create: d_model 256, 4 x 256 heads, window 1..128, 1..8 layers, either kind. */
int egoego_s1_train_ctx_create(const egoego_s1_config* cfg, int device, egoego_s1_train_ctx** out);
void egoego_s1_train_ctx_destroy(egoego_s1_train_ctx* ctx);
/* 0 (egoego_s1_train_last_error() says why) for a shape no call accepts. */
size_t egoego_s1_train_workspace_bytes(const egoego_s1_train_ctx* ctx, int n_windows);
size_t egoego_s1_train_saves_bytes(const egoego_s1_train_ctx* ctx, int n_windows);
/* d_feats [W][window][d_feats] fp32 and d_valid int32 [W] as for egoego_s1_encode (rows past valid[w] are read as zero rows,
 * whatever they hold) -> d_heads [W][window][4] (va | dist, HeadNet) or [W][3] (GravityNet, from token 0 of each window).
 * d_window_ids int64 [W] or NULL (window w has id w): the dropout streams; p_drop = 0: no dropout. */
int egoego_s1_train_forward(egoego_s1_train_ctx* ctx, const egoego_s1_weights* w, const float* d_feats, const int32_t* d_valid,
                            float p_drop, uint64_t dropout_seed, const int64_t* d_window_ids, int n_windows, void* d_saves,
                            size_t saves_bytes, void* d_workspace, size_t workspace_bytes, float* d_heads, void* stream);
/* From the saves of the forward call with the same weights, p_drop, dropout_seed and n_windows, and any upstream gradient
 * d_dheads of d_heads' shape: the gradient of every buffer of `grads` (overwritten). */
int egoego_s1_train_backward(egoego_s1_train_ctx* ctx, const egoego_s1_weights* w, const void* d_saves, size_t saves_bytes,
                             const float* d_dheads, const egoego_s1_train_grads* grads, float p_drop, uint64_t dropout_seed,
                             int n_windows, void* d_workspace, size_t workspace_bytes, void* stream);
/* The mask (1 keep / 0 drop, one byte each) a forward call with these arguments applies at `site` (EGOEGO_TRAIN_SITE_*) of `layer`:
 * site 0 [W][4][window][window], sites 1 and 2 [W][window][256].  The workspace holds the implied ids when d_window_ids is NULL. */
int egoego_s1_train_dropout_mask(egoego_s1_train_ctx* ctx, float p_drop, uint64_t dropout_seed, int layer, int site,
                                 const int64_t* d_window_ids, int n_windows, uint8_t* d_out, void* d_workspace, size_t workspace_bytes,
                                 void* stream);
/* Test/debug: copies saved tensor `which` of `layer` out of the saves of a forward call. */
int egoego_s1_train_saved(egoego_s1_train_ctx* ctx, const void* d_saves, size_t saves_bytes, int n_windows, int layer, int which,
                          float* d_out, void* stream);

/* HeadNet's loss and its gradient with respect to the heads, fp64 on fp32 inputs, no context: d_heads [B][window][4] (va | dist)
 * of which the first T <= window <= 128 rows of each sequence count; d_head_pose [B][T + 1][7] (xyz, quaternion w,x,y,z);
 * d_head_vels [B][T][6] (its last three columns are the angular velocity).  With q_0 = head_pose[b][0][3:] and
 * q_{t+1} = normalize(standardize(axis_angle_to_quaternion(quaternion_apply(q_t, va_t) / 30) (x) q_t)) (pytorch3d's formulas; q_t is
 * a constant of step t, as va2rot detaches it):
 *   orient = mean sum((|standardize(gt_{t+1} (x) conj(q_{t+1}))| - [1,0,0,0])^2),  va = mean |head_vels[..., 3:] - va|^2,
 *   dist = mean (dist - dist_scale |trans_{t+1} - trans_t|)^2, every mean over all B * T frames;
 *   d_loss[4] = (w_rotation orient + w_va va + w_dist dist, orient, va, dist)
 *   d_dheads64 / d_dheads (fp64 / fp32, either may be NULL) [B][window][4] = d(total) / d(heads), rows t >= T zero.
 * One workgroup per sequence walks the chain once; frame t's term and its gradient with respect to va_t come from one forward-mode
 * evaluation.  Sums: a fixed tree over a sequence's frames, then the sequences in order.  The workspace
 * (egoego_s1_headnet_loss_workspace_bytes, 256-byte aligned) may hold anything on entry. */
size_t egoego_s1_headnet_loss_workspace_bytes(int B);
int egoego_s1_headnet_loss(const float* d_heads, int window, int B, int T, const float* d_head_pose, const float* d_head_vels,
                           double dist_scale, double w_rotation, double w_va, double w_dist, double* d_loss, double* d_dheads64,
                           float* d_dheads, void* d_workspace, size_t workspace_bytes, void* stream);

/* ==================================================================================================================
 * GravityNet's training batches (egoego_s1_gravity_batch; added under ABI 8, purely additive): AMASSHeadPoseDataset.__getitem__
 * with augment_traj (amass_headpose_dataset.py:38-76, 115-165) for the B samples of a batch in ONE launch on `stream`: no
 * allocation, no host copy, no synchronisation, no workspace; every output is the caller's and is written whole.
 *   d_pose [n_rows][7] fp32 (xyz, quaternion w,x,y,z): the head poses of a split's n_seqs sequences, packed; d_offsets int32
 *   [n_seqs + 1]: sequence k is rows offsets[k] .. offsets[k + 1] - 1; d_seq_ids int32 [B]: the sequence of each sample;
 *   d_draw_ids int64 [B]: a sample's draws are a function of (seed, draw id) alone.
 * With len the sequence's rows and W = window: len - W - 1 <= 0 -> start 0, n = len frames; else n = W + 1 and start = 0 under
 * for_eval, else (word * (len - W - 1)) >> 32.  Rr = quaternion_to_matrix(o / copysign(|o|, o_0)) of four normals o, rounded to
 * fp32; s = 0.1 + 9.9 (word + 0.5) 2^-32 formed in fp64 and rounded to fp32.  The draws are Philox4x32-10 keyed by `seed` at the
 * counters (draw id low, draw id high, 0: the normals | 1: word 0 the start, word 1 the scale, 0x47424154); dropout and the sampler's
 * noise keep word 3 below 1000, so no counter of theirs coincides.  d_start int32 [B], d_rot fp32 [B][9], d_scale fp32 [B]: planted
 * draws, each NULL for "draw it".  Arithmetic fp64 on the fp32 inputs, each output rounded once:
 *   d_ori_head_pose [B][W + 1][7] the window's rows as they are; d_head_rot_mat [B][W + 1][3][3] = Rr R(q_t) (two_s = 2 / |q|^2);
 *   d_head_trans [B][W + 1][3] = s Rr (p_t - p_0) (the reference's serial sum of scaled differences, telescoped); rows n .. W of
 *   these three are zero; d_seq_len int32 [B] = n; d_aligned_rot_mat [B][3][3] = Rr^T; d_aligned_scale [B] = 1 / s (divided in
 *   fp64); d_floor_normal [B][3] = Rr[:, 2]; d_start_t_idx int32 [B] and d_aug_scale [B]: the start and s used.
 * A sample whose sequence id, offsets or planted start do not describe rows inside d_pose is written as an empty sample (n = 0,
 * all rows zero); nothing outside the arrays is read.  EGOEGO_E_INVALID before any launch: window < 1, B < 1, n_rows < 1,
 * n_seqs < 1, a NULL pointer other than the three planted draws.  egoego_s1_data_last_error() describes the last failure.
 * ================================================================================================================== */
const char* egoego_s1_data_last_error(void);
int egoego_s1_gravity_batch(const float* d_pose, int n_rows, const int32_t* d_offsets, int n_seqs, const int32_t* d_seq_ids,
                            const int64_t* d_draw_ids, int B, int window, uint64_t seed, int for_eval, const int32_t* d_start,
                            const float* d_rot, const float* d_scale, float* d_ori_head_pose, float* d_head_rot_mat, float* d_head_trans,
                            int32_t* d_seq_len, float* d_aligned_rot_mat, float* d_aligned_scale, float* d_floor_normal,
                            int32_t* d_start_t_idx, float* d_aug_scale, void* stream);

/* HeadNet's training batches (egoego_s1_head_batch; added under ABI 8, purely additive): ARESHeadPoseDataset.__getitem__
 * (ares_headpose_dataset.py:270-333, shared by the GIMO and real-world datasets) for the B samples of a batch in ONE launch on
 * `stream`: no allocation, no host copy, no synchronisation, no workspace; every output is the caller's and is written whole.
 * Nothing is computed: every output word is a copy of a table's word or a zero.  All tables and outputs are 16-byte aligned.
 *   d_pose [n_rows][7], d_vels [n_rows][6] fp32 and d_offsets int32 [n_seqs + 1]: sequence k is rows offsets[k] .. offsets[k + 1]
 *   - 1 (T_k of them); d_feats [n_rows - n_seqs][D] fp32: its F_k = T_k - 1 feature rows start at row offsets[k] - k; D a multiple
 *   of 4.  Optional, NULL together: d_slam32 [n_slam_rows][29] fp32 (aligned trans 3 | aligned quat 4 | aligned rot 9 | original
 *   quat 4 | original rot 9), d_slam_trans64 [n_slam_rows][3] fp64 (the original translation, not rounded) and d_slam_offsets int32
 *   [n_seqs + 1] (L_k rows of sequence k).  d_seq_ids int32 [B], d_draw_ids int64 [B], d_start int32 [B] (planted starts) or NULL.
 * The window, W = window: training has room = F_k - W + 1, n = W and start = (word 0 * room) >> 32 of Philox4x32-10 keyed by `seed`
 * at the counter (draw id low, draw id high, 1, 0x48424154) (egoego_s1_gravity_batch's counters hold 0x47424154 there, dropout and
 * the sampler's noise a number below 1000), or the planted start; for_eval has start = 0 (d_start is not read) and n = min(F_k, W).
 *   d_head_pose [B][W + 1][7]: rows start .. start + n, rows > n zero; d_head_vels [B][W][6] and d_of [B][W][D]: rows start ..
 *   start + n - 1, rows >= n zero; d_seq_len int32 [B] = n; d_start_t_idx int32 [B].  With the SLAM tables, the seven SLAM outputs
 *   (NULL together, and with the tables): d_aligned_slam_trans [B][W + 1][3], d_aligned_slam_rot_quat [..][4], d_aligned_slam_rot_mat
 *   [..][9], d_ori_slam_trans fp64 [..][3], d_ori_slam_rot_quat [..][4], d_ori_slam_rot_mat [..][9]: rows start .. of the track,
 *   d_pose_len int32 [B] = clamp(L_k - start, 0, n + 1) of them, the rest zero.
 * An EMPTY sample (seq_len 0, pose_len 0, start 0, every row zero) is written where the sequence id or its offsets do not describe
 * rows inside the tables, where F_k < 1, where room < 1 in training, and where a planted start is outside 0 .. room - 1; nothing
 * outside the tables is read.  EGOEGO_E_INVALID before any launch: window < 1, B < 1, D < 4 or D % 4 != 0, n_rows < 1, n_seqs < 1,
 * a NULL required pointer, the SLAM tables or outputs given in part or one group without the other. */
int egoego_s1_head_batch(const float* d_pose, const float* d_vels, const float* d_feats, int n_rows, int d_feats_dim,
                         const int32_t* d_offsets, int n_seqs, const float* d_slam32, const double* d_slam_trans64,
                         const int32_t* d_slam_offsets, int n_slam_rows, const int32_t* d_seq_ids, const int64_t* d_draw_ids, int B,
                         int window, uint64_t seed, int for_eval, const int32_t* d_start, float* d_head_pose, float* d_head_vels,
                         float* d_of, int32_t* d_seq_len, int32_t* d_start_t_idx, float* d_aligned_slam_trans,
                         float* d_aligned_slam_rot_quat, float* d_aligned_slam_rot_mat, double* d_ori_slam_trans,
                         float* d_ori_slam_rot_quat, float* d_ori_slam_rot_mat, int32_t* d_pose_len, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGOEGO_HIP_H */

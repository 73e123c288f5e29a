/*
 * mappo_hip.h -- C ABI of libmappo_hip.so: the MI355X (gfx950) device side of the
 * MAPPO rollout-buffer hot path (GAE scan, advantage moments, minibatch gathers,
 * slab writes).
 *
 * The reference (marlbenchmark/on-policy) has no FFI for this path: it is numpy
 * code inside onpolicy/utils/shared_buffer.py and onpolicy/algorithms/r_mappo/r_mappo.py.
 * Each entry point below names the reference lines it replaces.  A maintainer binds
 * them with ctypes; no torch / C++ types cross this boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the comment says "host";
 *   - all payload is float32, C-contiguous, time-major: element (t, n, a, d) of a
 *     field with row width D lives at ((t*N + n)*A + a)*D + d; "C" below is the
 *     number of columns N*A of the [T(+1), C] scalar fields;
 *   - the library borrows pointers for the duration of the call and allocates
 *     nothing persistent; work is enqueued on `stream` (a hipStream_t) and the call
 *     returns without synchronising;
 *   - return value: 0 on success, a negative MAPPO_E_* for argument errors (nothing
 *     enqueued), or a positive hipError_t from the launch.
 */
#ifndef MAPPO_HIP_H
#define MAPPO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mappo_stream_t; /* hipStream_t; NULL = the null stream */

#define MAPPO_ABI_VERSION 2

/* argument errors */
#define MAPPO_E_NULL      (-1) /* a required pointer is NULL                */
#define MAPPO_E_SHAPE     (-2) /* a size is <= 0 or inconsistent            */
#define MAPPO_E_FLAGS     (-3) /* unsupported flag combination              */
#define MAPPO_E_TOO_MANY  (-4) /* more fields / slabs than MAPPO_MAX_FIELDS */
#define MAPPO_E_ALIGN     (-5) /* a pointer is not 4-byte aligned           */

/* Arithmetic of the matrix products of K9 / K12 (field `arith` of mappo_mlp_t / mappo_gru_seq_t; a PER-CALL choice, nothing
 * process-wide: two trainers in one process may differ).  Inputs, outputs, accumulation and every non-matrix operation are
 * float32 in both forms.
 *   MAPPO_ARITH_SIX_TERM (0, what a zero-initialised struct selects): wherever a kernel of that form exists -- the forward of
 *     two-layer trunks with aligned inputs, the backward chain of two-layer trunks, the direct first-layer weight-gradient
 *     kernel (aligned inputs wider than 192 floats), both directions of K12 -- every float32 product x y is formed on the
 *     bf16 matrix cores (v_mfma_f32_32x32x16_bf16, 16 x the rate of the float32 instruction) from the operands' EXACT
 *     three-way bf16 splits x = x1 + x2 + x3 (8 + 8 + 8 significand bits, round-to-nearest, residuals exact):
 *     x y ~ x1 y1 + (x1 y2 + x2 y1) + (x2 y2 + x1 y3 + x3 y1), six products that are exact in float32, accumulated in
 *     float32 smallest first; the three dropped terms are < 2^-23 |x y| together (profiles/r04_probe_bf16_split.json, r05
 *     adversarial tests: the error against float64 is of the float32 MFMA chain's order, bounded by a few 2^-23 sum|x||y|).
 *     Shapes without such a kernel (single- / three-layer trunks, unaligned or very narrow weight-gradient shapes) run the
 *     float32-MFMA kernels under either value.  NON-FINITE AND OUT-OF-RANGE OPERANDS: an operand that is +-inf, NaN or so
 *     large that its bf16 rounding overflows (|x| >= 3.3961e38) makes every output it reaches NaN (inf - inf in the split)
 *     -- a superset of where the float32 form is non-finite (which yields +-inf / NaN, or, behind a saturating Tanh on raw
 *     inputs, finite values); a non-finite loss / gradient norm poisons the update identically in both forms
 *     (mappo_clip_adam).  Float32 subnormal operands are split inexactly (bf16 keeps 7 of their bits per part): absolute
 *     error <= 2^-133 |y| per product.
 *   MAPPO_ARITH_F32_MFMA (1): v_mfma_f32_32x32x2_f32 everywhere (exact float32 fma chains). */
#define MAPPO_ARITH_SIX_TERM 0
#define MAPPO_ARITH_F32_MFMA 1

/* ---------------------------------------------------------------- K1: GAE ----
 * Replaces SharedReplayBuffer.compute_returns
 *   (onpolicy/utils/shared_buffer.py:179-262) and, when `advantages` is given, the
 *   first line of R_MAPPO.train (onpolicy/algorithms/r_mappo/r_mappo.py:179-182).
 *
 * flags select the reference branch:
 *   USE_GAE              args.use_gae                 (shared_buffer.py:186,217)
 *   PROPER_TIME_LIMITS   args.use_proper_time_limits  (shared_buffer.py:185)
 *   DENORM               use_popart or use_valuenorm: D(x) = x*sigma + mu with
 *                        (sigma, mu) = denorm[0..1]    (valuenorm.py:68-79,
 *                        popart.py:88-98); without it D is the identity.
 * gamma and gae_lambda are the Python floats (float64) of args.gamma /
 * args.gae_lambda: the reference multiplies gamma*gae_lambda in float64 and only then
 * rounds to float32 (shared_buffer.py:239), and so does this call.
 * Arithmetic is float32 in exactly the reference's operation order, with no FMA
 * contraction, so results are bit-identical to the numpy path given the same
 * (sigma, mu) -- with one exception: narrow buffers in the GAE modes (2048 <= C < 16384
 * columns, 64 <= T <= 416) run a TIME-PARALLEL scan (the recurrence is affine in the
 * accumulator, T is cut into 16 segments that are folded independently and stitched by
 * composing their affine maps; the serial walk otherwise leaves such buffers at < 10 % of
 * HBM bandwidth).  Inside a segment the operations are the reference's, the 15 segment
 * boundaries carry a few ulp of re-association error: results agree to ~1e-6 relative, the
 * "fp32 tolerance" of BASELINE.json's north star.  MAPPO_GAE_EXACT forces the bit-exact
 * kernels for every shape.
 *
 *   rewards      [T,   C]  read
 *   value_preds  [T+1, C]  read; row T is first overwritten with next_value in the
 *                          GAE modes (shared_buffer.py:187,218)
 *   next_value   [C]       read
 *   masks        [T+1, C]  read (rows 1..T)
 *   bad_masks    [T+1, C]  read (rows 1..T); required iff PROPER_TIME_LIMITS
 *   returns      [T+1, C]  rows 0..T-1 written; row T is written (= next_value)
 *                          only in the non-GAE modes (shared_buffer.py:205,260)
 *   denorm       [2]       {sigma, mu}; required iff DENORM
 * Optional fused epilogue (all three NULL to skip):
 *   advantages   [T, C]    advantages[t] = fl(returns[t] - D(value_preds[t]))
 *                          (r_mappo.py:179-182: computed from the ROUNDED returns)
 *   active_masks [T+1, C]  rows 0..T-1 select the entries that count towards the
 *                          moments (r_mappo.py:184: active_masks[:-1] == 0 -> NaN);
 *                          NULL = every entry counts
 *   adv_partials [mappo_gae_partial_rows(C), 3] float64; per-workgroup partial
 *                          {sum adv, sum adv^2, count} over counted entries; rows
 *                          that no workgroup owns are zero-filled by this call.
 */
#define MAPPO_GAE_USE_GAE            1u
#define MAPPO_GAE_PROPER_TIME_LIMITS 2u
#define MAPPO_GAE_EXACT              8u   /* never take the time-parallel scan (see below): bit-identical results */
#define MAPPO_GAE_DENORM             4u

int mappo_gae_f32(const float* rewards, float* value_preds, const float* next_value,
                  const float* masks, const float* bad_masks, float* returns,
                  const float* denorm, float* advantages, const float* active_masks,
                  double* adv_partials, int T, int64_t C, double gamma, double gae_lambda,
                  unsigned flags, mappo_stream_t stream);

/* Multi-agent-transformer branches of SharedReplayBuffer.compute_returns (shared_buffer.py:222-232
 * with a value normaliser, :241-251 without; taken when args.algorithm_name is "mat" / "mat_dec",
 * use_gae is set and use_proper_time_limits is not).  Same storage contract as mappo_gae_f32 with
 * C = n_rollout_threads * num_agents columns ordered (thread, agent); differences:
 *   advantages [T, C]  REQUIRED: advantages[t] = the GAE accumulator itself (:231,:250), which is
 *                      what MATTrainer.train normalises (mat_trainer.py:160-164);
 *   flags              MAPPO_GAE_DENORM: delta uses each agent's own D(v) (:223-229);
 *                      0: delta uses the float32 mean over the env's num_agents agents of the raw
 *                      value predictions, summed in numpy's pairwise order (:243-245), and
 *                      returns[t] = gae + value_preds[t] of the agent itself (:251);
 *                      num_agents <= 128 in this mode (MAPPO_E_TOO_MANY otherwise).
 * adv_partials / active_masks as in mappo_gae_f32 (moments of the advantages written). */
int mappo_gae_mat_f32(const float* rewards, float* value_preds, const float* next_value,
                      const float* masks, float* returns, const float* denorm, float* advantages,
                      const float* active_masks, double* adv_partials, int T, int64_t C,
                      int num_agents, double gamma, double gae_lambda, unsigned flags,
                      mappo_stream_t stream);

/* Number of [.,3] float64 rows mappo_gae_f32 / mappo_advantages_f32 need in adv_partials
 * for C columns. */
int64_t mappo_gae_partial_rows(int64_t C);

/* Standalone form of the fused epilogue above, for callers whose returns / value_preds /
 * normaliser changed after mappo_gae_f32 ran (r_mappo.py:179-186):
 *   advantages[i] = fl(returns[i] - D(value_preds[i])), i < T*C, plus the same partial
 *   moments. denorm NULL = identity, active_masks NULL = every entry counts. */
int mappo_advantages_f32(const float* returns, const float* value_preds, const float* denorm,
                         const float* active_masks, float* advantages, double* adv_partials,
                         int T, int64_t C, mappo_stream_t stream);

/* Tuning hook for benchmarks: selects the kernel used by mappo_gae_f32 (0 = automatic).  variant % 1000 names the kernel:
 * 36, 54, 56, 57 = the four LDS-DMA ring shapes the automatic choice picks from, 70 = the time-parallel scan (71 and 72,
 * scan widths that are no longer built, are aliases of 70), 99 = one lane per column.  Any other number has no kernel
 * of its own and runs the one-lane-per-column kernel.  variant / 1000 carries option bits for the ring kernels:
 * 1 = XCD-contiguous strip order, 2 = non-temporal DMA loads (the automatic choice sets both).  All of them but the scan
 * produce bit-identical results.  Returns the previous value. */
int mappo_gae_set_variant(int variant);

/* The variant the most recent mappo_gae_f32 call of this process launched (0 before the first call):
 * 70 = the time-parallel scan (tolerance mode), 99 = one lane per column, 36 / 54 / 56 / 57 the bit-exact
 * LDS-DMA ring kernels (a number without a kernel of its own is reported as given and ran one lane per column).  For tests that must know which arithmetic a shape took. */
int mappo_gae_last_variant(void);

/* Measurement hook for benchmarks: mappo_gae_time_next_launch arms one of 64 slots (returned, >= 0; they are reused in a ring)
 * and the NEXT LDS-DMA ring launch of mappo_gae_f32 in this process (every GAE-mode call with aligned columns; not the
 * one-lane-per-column kernel, not the scan) is bracketed by that slot's HIP event pair at dispatch level
 * (hipExtLaunchKernelGGL: kernel begin / end timestamps, what rocprofv3 --kernel-trace reports), on the stream of that call.
 * mappo_gae_timed_launch_ms(slot) waits for that launch and returns its duration in milliseconds; MAPPO_E_FLAGS if the slot
 * was never armed or its armed call launched a kernel without the hook.  (A pair of hipEventRecord calls around a launch also
 * times two packets of the command processor: + 5-6 us on this 50 us kernel.)  Not thread-safe, like the other hooks. */
int mappo_gae_time_next_launch(void);
int mappo_gae_timed_launch_ms(int slot, float* ms);

/* --------------------------------------------- K5: advantage moments / stats ----
 * Replaces np.nanmean / np.nanstd over the masked advantages
 *   (onpolicy/algorithms/r_mappo/r_mappo.py:183-186).
 * mappo_adv_reduce:  sums[0..2] = column sums of partials[rows,3], fixed order
 *                    (deterministic). In a multi-GPU job the caller all-reduces
 *                    `sums` (3 float64) across ranks between the two calls.
 * mappo_adv_stats:   stats[0] = mean = S1/n, stats[1] = population std
 *                    = sqrt(max(S2/n - mean^2, 0)), both rounded to float32.
 * The normalisation (adv - mean) / (std + 1e-5) (r_mappo.py:187) is applied by the
 * gather kernels (field.normalize) so no standalone pass over [T,C] is needed.
 */
int mappo_adv_reduce(const double* partials, int64_t rows, double* sums, mappo_stream_t stream);
int mappo_adv_stats(const double* sums, float* stats, mappo_stream_t stream);

/* Standalone normalisation pass, for callers that want the normalised advantages
 * materialised (out may alias adv): out = (adv - stats[0]) / (stats[1] + 1e-5f). */
int mappo_adv_normalize(const float* adv, const float* stats, float* out, int64_t n,
                        mappo_stream_t stream);

/* ------------------------------------------------- K3 / K4: minibatch gathers ----
 * One launch copies a minibatch of rows of up to MAPPO_MAX_FIELDS buffer fields.
 *
 * mappo_gather_rows replaces the per-minibatch fancy indexing of
 *   SharedReplayBuffer.feed_forward_generator (shared_buffer.py:363-396):
 *   dst_f[j, :] = src_f[idx[j], :],  j in [0, mb), rows in (t, n, a) order.
 *
 * mappo_gather_chunks replaces recurrent_generator (shared_buffer.py:499-608,
 *   helpers _cast :11-12, _flatten :7-8) and, with L == T, naive_recurrent_generator
 *   (:402-497), reading straight from the time-major buffer (no transposed copy):
 *   output row (l, j) -> flat f = idx[j]*L + l of the (n, a, t)-ordered view,
 *   n = f / (A*T), a = (f / T) % A, t = f % T, source row (t*N + n)*A + a;
 *   dst_f[l*mb + j, :] = src_f[that row, :].  Fields with first_only != 0 (the RNN
 *   states, shared_buffer.py:568-569,588-589) take only l = 0: dst_f[j, :].
 *   A chunk may straddle two (n, a) trajectories when T % L != 0, exactly as the
 *   reference does.
 *
 * fields is a HOST array; idx is a DEVICE int64 array; stats (device, {mean, std})
 * is required iff some field has normalize != 0.
 */
#define MAPPO_MAX_FIELDS 16

typedef struct mappo_field {
    const float* src;   /* field base (row 0), rows of `width` floats          */
    float*       dst;   /* output base, contiguous rows of `width` floats      */
    int32_t      width; /* floats per row (> 0)                                */
    int32_t      first_only; /* chunk gather only: copy the l = 0 row per chunk */
    int32_t      normalize;  /* dst = (src - stats[0]) / (stats[1] + 1e-5f)     */
    int32_t      standardize; /* dst row = (row - mean(row)) / sqrt(var(row) + 1e-5): the parameter-free
                                 part of the input nn.LayerNorm (ref algorithms/utils/mlp.py:47-53),
                                 applied while the row is copied; widths as for mappo_layernorm_fwd */
} mappo_field_t;

int mappo_gather_rows(const mappo_field_t* fields, int n_fields, const int64_t* idx,
                      int64_t mb, const float* stats, mappo_stream_t stream);

int mappo_gather_chunks(const mappo_field_t* fields, int n_fields, const int64_t* idx,
                        int64_t mb, int L, int T, int64_t N, int A, const float* stats,
                        mappo_stream_t stream);

/* Packed records of the NARROW fields.  A 4-byte gather costs a whole HBM sector, so the per-sample
 * scalars of feed_forward_generator / recurrent_generator (actions, value_preds, returns, masks,
 * active_masks, action_log_probs, advantages, and small rows such as available_actions;
 * shared_buffer.py:383-396, 558-566) are first packed into one record per (t, n, a) row:
 *   mappo_pack_records:   records[row, offset_k .. offset_k + width_k) = src_k[row, :], rows in
 *                         (t, n, a) order; record_width a multiple of 4, <= 32; padding zeroed.
 *   mappo_gather_records: dst_k[j, :] = records[source_row(j), offset_k ..] (normalised like
 *                         mappo_field.normalize if asked) -- one record read per sample.
 *                         L = 0: rows mode (source_row(j) = idx[j]); L > 0: chunk mode with the row
 *                         mapping of mappo_gather_chunks (no first_only fields here).
 * Bit-identical to gathering the fields one by one.  `fields` is a HOST array. */
typedef struct mappo_record_field {
    const float* src;    /* pack: field base (rows of `width` floats); unused by gather          */
    float*       dst;    /* gather: output base (rows of `width` floats); unused by pack         */
    int32_t      width;
    int32_t      offset; /* first component of this field inside a record                        */
    int32_t      normalize;
    int32_t      reserved;
} mappo_record_field_t;

int mappo_pack_records(const mappo_record_field_t* fields, int n_fields, float* records,
                       int record_width, int64_t rows, mappo_stream_t stream);
int mappo_gather_records(const float* records, int record_width, const mappo_record_field_t* fields,
                         int n_fields, const int64_t* idx, int64_t mb, int L, int T, int64_t N, int A,
                         const float* stats, mappo_stream_t stream);

/* Tuning hook for benchmarks (results do not depend on it): bits 4.. are the workgroups per CU of the
 * gathers' persistent grid (0 = what occupancy allows).  The low four bits once selected the loads in
 * flight per lane and non-temporal access; the one shape that is built has two loads in flight and
 * non-temporal accesses, and those bits are accepted and ignored.  The default is 5.  Returns the
 * previous value.  Not thread-safe, like the other hooks. */
int mappo_gather_set_variant(int variant);

/* ------------------------------------------------------------ K2: slab writes ----
 * Replaces the per-field `buf[step] = x.copy()` statements of insert / chooseinsert /
 * after_update / chooseafter_update (shared_buffer.py:107-121,142-156,162-170,
 * 174-177): one launch copies up to MAPPO_MAX_FIELDS contiguous [N, A, D] slabs
 * (device to device).  slabs is a HOST array.
 */
typedef struct mappo_slab {
    const float* src;
    float*       dst;
    int64_t      count; /* floats */
} mappo_slab_t;

int mappo_slab_copy(const mappo_slab_t* slabs, int n_slabs, mappo_stream_t stream);

/* The same launch + the slabs of row-standardised observation copies that have to follow the slabs being written (round 6).
 * Networks with an input LayerNorm (reference onpolicy/algorithms/utils/mlp.py:47-53: feature_norm) read obs / share_obs
 * through a resident copy whose rows hold (x - mean) / sqrt(var + eps) (mappo_standardize_rows_ld; the LayerNorm's affine half
 * is folded into the first Linear); when insert / chooseinsert / after_update (shared_buffer.py:90-177) rewrite a slab of the
 * field, the same slab of the copy is recomputed from the VALUE being written -- by extra workgroups of this launch, in the
 * layout mappo_standardize_rows_ld writes (its arithmetic is this function's own, see below: the rows agree with
 * mappo_standardize_rows_ld to rounding, not bit for bit).  src [rows, D] floats; dst [rows, ld >= D] floats, columns
 * D .. ld - 1 are written as zeros.  std is a HOST array of at most MAPPO_MAX_STD_SLABS entries; n_std = 0 is
 * mappo_slab_copy; n_slabs = 0 (slabs may be NULL) only standardises -- the full pass over a field goes through here too, so
 * that slab and full pass are one piece of code (every operation IEEE, one explicit fused multiply-add per term of the
 * second moment) and bit-identical to each other by construction (tests/test_gpu_standardize_at_insert.py). */
#define MAPPO_MAX_STD_SLABS 4
typedef struct mappo_std_slab {
    const float* src;
    float*       dst;
    int64_t      rows;
    int          D, ld;
    float        eps;
} mappo_std_slab_t;

int mappo_slab_copy_std(const mappo_slab_t* slabs, int n_slabs, const mappo_std_slab_t* std, int n_std,
                        mappo_stream_t stream);

/* ------------------------------------------------------------ K6: row LayerNorm ----
 * The LayerNorm the reference applies to the observations and after every Linear / GRU of the
 * actor and critic trunks (onpolicy/algorithms/utils/mlp.py:17-22,47-53, rnn.py:22,79:
 * nn.LayerNorm over the last dimension, eps = 1e-5, biased variance), as one streaming kernel per
 * direction for [M, D] float32 rows with D up to 2048 (multiple of 4) / 1536 (any).
 *
 * mappo_layernorm_fwd: y = (x - mean) * rstd * weight + bias; also writes mean[M], rstd[M]
 *                      (saved for the backward).
 * mappo_layernorm_bwd: dx (NULL to skip: input does not require grad), dweight[D], dbias[D] from
 *                      dy, x and the saved statistics.  `partials` is a device workspace of
 *                      2 * mappo_layernorm_max_blocks() * D floats (per-workgroup column sums,
 *                      reduced in a fixed order: deterministic).
 * Returns MAPPO_E_SHAPE for an unsupported D (callers then use the framework's own LayerNorm).
 */
/* mappo_act_layernorm_fwd/_bwd: the same with an elementwise activation fused in front,
 * y = LayerNorm(act(x)), act: 0 = identity, 1 = tanh, 2 = relu -- one pass over the rows instead of
 * two for the `Linear -> act -> LayerNorm` blocks of mlp.py:17-22.  `x` is the PRE-activation in
 * both directions (the backward recomputes act(x)); dx is the gradient w.r.t. the pre-activation.
 */
/* mappo_bias_act_layernorm_fwd/_bwd: additionally the bias add of the preceding Linear,
 * y = LayerNorm(act(x + pre_bias)) with pre_bias [D] (NULL = 0): the GEMM runs without a bias and the
 * backward returns dpre_bias [D] = column sums of dx, i.e. the Linear's bias gradient, for free --
 * otherwise a separate pass over the [M, D] gradient (mlp.py:17-22 `nn.Linear` + `nn.LayerNorm`).
 * `partials` is 3 * mappo_layernorm_max_blocks() * D floats when dpre_bias is requested (D <= 1024,
 * dx required), 2 * ... otherwise. */
int mappo_layernorm_max_blocks(void);
/* Which kernel shape the LayerNorm launchers and the standardising gather (mappo_field.standardize) take for rows of D
 * floats: vec | lpr << 8 | epl << 16 (vec floats per access, lpr lanes per row, epl accesses per lane; a workgroup
 * covers 256 / lpr rows per trip of its row loop), or 0 for a width they refuse with MAPPO_E_SHAPE.  aligned16 != 0:
 * every operand starts on a 16-byte boundary; 0: some operand does not (float accesses, D <= 1536).  A host query:
 * takes no pointers, launches nothing. */
int mappo_layernorm_shape(int D, int aligned16);
int mappo_bias_act_layernorm_fwd(const float* x, const float* pre_bias, const float* weight, const float* bias,
                                 float* y, float* mean, float* rstd, int64_t M, int D, float eps, int act,
                                 mappo_stream_t stream);
int mappo_bias_act_layernorm_bwd(const float* dy, const float* x, const float* pre_bias, const float* mean,
                                 const float* rstd, const float* weight, float* dx, float* dweight, float* dbias,
                                 float* dpre_bias, float* partials, int64_t M, int D, int act,
                                 mappo_stream_t stream);
int mappo_act_layernorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean,
                            float* rstd, int64_t M, int D, float eps, int act, mappo_stream_t stream);
int mappo_act_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                            const float* weight, float* dx, float* dweight, float* dbias, float* partials,
                            int64_t M, int D, int act, mappo_stream_t stream);
int mappo_layernorm_fwd(const float* x, const float* weight, const float* bias, float* y, float* mean,
                        float* rstd, int64_t M, int D, float eps, mappo_stream_t stream);
int mappo_layernorm_bwd(const float* dy, const float* x, const float* mean, const float* rstd,
                        const float* weight, float* dx, float* dweight, float* dbias, float* partials,
                        int64_t M, int D, mappo_stream_t stream);

/* --------------------------------------------------------------- K7: fused PPO loss ----
 * The clipped-surrogate loss of R_MAPPO.ppo_update for a Discrete action head, value and gradient in
 * one pass over the rows of a minibatch (r_mappo.py:52-89 cal_value_loss, :119-153 policy loss and
 * entropy; act.py:115-170 and distributions.py FixedCategorical for log-prob / entropy of the masked
 * logits).  Per row i (all arrays float32, row-major):
 *   logits [rows, n_actions]  raw outputs of the action head; available [rows, n_actions] (NULL = all
 *   available; entries == 0 take logit -1e10 and receive zero gradient); actions [rows] (index as
 *   float); old_logp, adv, active (NULL = 1), factor (NULL = 1; HAPPO, happo_trainer.py:137-141),
 *   values, value_preds, returns [rows]; norm = {sigma, mu} of the value normaliser, the layout of
 *   mappo_gae_f32's denorm: target = (returns - mu) / sigma (NULL = raw returns); inv_denoms = {1 / D_policy, 1 / D_value} device scalars -- the denominators of the
 *   masked means (sum of active masks, or the row count) over the WHOLE minibatch (all spans, all
 *   data-parallel ranks), so that the gradients of successive spans simply accumulate.
 * Outputs: dlogits [rows, n_actions] = d(policy_loss - entropy_coef * entropy) / dlogits,
 *          dvalues [rows] = d(value_loss_coef * value_loss) / dvalues (either may be NULL),
 *          sums[4] += { sum w_p * (-surrogate), sum w_p * entropy, sum w_v * value_loss, sum ratio }
 *          (float64, atomically accumulated: multiply by inv_denoms for the logged means).
 * logits == NULL skips the actor half, values == NULL the critic half. */
#define MAPPO_LOSS_HUBER               1u  /* args.use_huber_loss (else mse) */
#define MAPPO_LOSS_CLIPPED_VALUE       2u  /* args.use_clipped_value_loss */
#define MAPPO_LOSS_POLICY_ACTIVE_MASKS 4u  /* args.use_policy_active_masks */
#define MAPPO_LOSS_VALUE_ACTIVE_MASKS  8u  /* args.use_value_active_masks */
typedef struct mappo_ppo_loss {
    const float* logits;
    const float* available;
    const float* actions;
    const float* old_logp;
    const float* adv;
    const float* active;
    const float* factor;
    const float* values;
    const float* value_preds;
    const float* returns;
    const float* norm;
    const float* inv_denoms;
    float* dlogits;
    float* dvalues;
    double* sums;
    int64_t rows;
    int n_actions;
    float clip;
    float huber_delta;
    float entropy_coef;
    float value_loss_coef;
    unsigned flags;
} mappo_ppo_loss_t;
int mappo_ppo_loss_f32(const mappo_ppo_loss_t* args, mappo_stream_t stream);

/* ------------------------------------------------------ K7 for MultiDiscrete heads: one launch for all sub-heads ----
 * The same loss for a MultiDiscrete action head (act.py, multi-discrete branch of evaluate_actions: one Categorical
 * per sub-head, no availability mask; r_mappo.py:119-153).  logits [rows, S] holds the sub-heads' raw outputs side by
 * side, S = sum of head_sizes; actions and old_logp are [rows, num_heads] (index as float; log-prob per sub-head).
 * Per row and sub-head h: logp_h from the log-softmax of the head's logits, ratio_h = exp(logp_h - old_logp_h),
 * surr_h = min(ratio_h * adv, clamp(ratio_h, 1 -+ clip) * adv).  The row's policy term is -sum_h surr_h; the entropy is
 * the mean over sub-heads of the per-head (masked) means, so the row's entropy term is sum_h H_h / num_heads.
 * adv, active (NULL = 1), values, value_preds, returns [rows], norm, inv_denoms, the scalars and the flags are those of
 * mappo_ppo_loss_f32; the value half is the same arithmetic.  Everything but active and norm is required.
 * Outputs: dlogits [rows, S] = d(policy_loss - entropy_coef * entropy) / dlogits, dvalues [rows],
 *          sums[4] += { sum w_p * (-sum_h surr_h), sum w_p * sum_h H_h / num_heads, sum w_v * value_loss,
 *                       sum (sum_h ratio_h / num_heads) }  (float64, atomically accumulated).
 * 1 <= num_heads <= MAPPO_LOSS_MULTI_MAX_HEADS, every head_sizes[h] >= 1, S <= 64 (the limits of
 * mappo_multi_categorical_sample); MAPPO_E_SHAPE otherwise. */
#define MAPPO_LOSS_MULTI_MAX_HEADS 8
typedef struct mappo_ppo_loss_multi {
    const float* logits;
    const float* actions;
    const float* old_logp;
    const float* adv;
    const float* active;
    const float* values;
    const float* value_preds;
    const float* returns;
    const float* norm;
    const float* inv_denoms;
    float* dlogits;
    float* dvalues;
    double* sums;
    int64_t rows;
    int num_heads;
    int head_sizes[MAPPO_LOSS_MULTI_MAX_HEADS];
    float clip;
    float huber_delta;
    float entropy_coef;
    float value_loss_coef;
    unsigned flags;
} mappo_ppo_loss_multi_t;
int mappo_ppo_loss_multi_f32(const mappo_ppo_loss_multi_t* args, mappo_stream_t stream);

/* ------------------------------------------------------------------ K14: categorical sampling for the rollout ----
 * Replaces, for one Discrete head and one draw per row, Categorical.forward's availability masking
 * (onpolicy/algorithms/utils/distributions.py:64-67), FixedCategorical.sample (:15-16) and .log_probs (:18-25) as
 * called by ACTLayer.forward (onpolicy/algorithms/utils/act.py:55-60):
 *   x_i = available_i == 0 ? -1e10 : logits_i;  l = x - logsumexp(x);  action = argmax_i exp(l_i) / noise_i
 *   (torch.multinomial's rule for one sample: noise ~ Exponential(1), drawn by the caller);  log_probs = l[action].
 *   logits [rows, n_actions], available [rows, n_actions] or NULL, noise [rows, n_actions] (> 0),
 *   actions [rows] int64, log_probs [rows]; n_actions <= 64. */
int mappo_categorical_sample(const float* logits, const float* available, const float* noise, int64_t* actions,
                             float* log_probs, int64_t rows, int n_actions, mappo_stream_t stream);

/* ------------------------------------------------------ K14 for MultiDiscrete heads: one launch for all sub-heads ----
 * ACTLayer.forward's multi-discrete branch (onpolicy/algorithms/utils/act.py) samples every sub-head as above (no
 * availability mask) and concatenates actions and log-probs.  logits [rows, sum_k head_sizes[k]] (the sub-heads'
 * logits side by side); noise: host array of num_heads device pointers, noise[k] [rows, head_sizes[k]] (> 0) -- the
 * Exponential(1) draws of sub-head k's torch.multinomial, drawn in head order; head_sizes: host array.  Outputs
 * actions [rows, num_heads] int64 and log_probs [rows, num_heads] (per sub-head, not summed).
 * num_heads <= MAPPO_MULTI_SAMPLE_MAX_HEADS, sum of head_sizes <= 64. */
#define MAPPO_MULTI_SAMPLE_MAX_HEADS 8
int mappo_multi_categorical_sample(const float* logits, const float* const* noise, const int* head_sizes,
                                   int num_heads, int64_t* actions, float* log_probs, int64_t rows,
                                   mappo_stream_t stream);

/* ------------------------------------------------- K14 mode: the deterministic action of a Categorical head ----
 * Replaces, for one Discrete head, Categorical.forward's availability masking
 * (onpolicy/algorithms/utils/distributions.py:64-67), FixedCategorical.mode (:27-28) and .log_probs (:18-25) as called
 * by ACTLayer.forward with deterministic=True (onpolicy/algorithms/utils/act.py:55-60):
 *   x_i = available_i == 0 ? -1e10 : logits_i;  action = the LOWEST i at which x_i is maximal (compared as float32:
 *   softmax is monotone, so this is the mode);  log_probs = x[action] - logsumexp(x), evaluated as
 *   -log(sum_i exp(x_i - x[action])): no rounding at the size of the logits.
 *   logits [rows, n_actions] (finite values only: a NaN or an infinity is outside the contract), available
 *   [rows, n_actions] or NULL, actions [rows] int64, log_probs [rows]; n_actions <= 64.
 * MAPPO_E_NULL / MAPPO_E_SHAPE are returned before anything touches the device. */
int mappo_categorical_mode(const float* logits, const float* available, int64_t* actions, float* log_probs,
                           int64_t rows, int n_actions, mappo_stream_t stream);

/* --------------------------------------------- K14 mode for MultiDiscrete heads: one launch for all sub-heads ----
 * ACTLayer.forward's multi-discrete branch with deterministic=True (onpolicy/algorithms/utils/act.py:44-60: per
 * sub-head FixedCategorical.mode / log_probs, distributions.py:14-28, then cat), no availability mask.
 * logits [rows, sum_k head_sizes[k]] (finite), head_sizes: host array.  Outputs actions [rows, num_heads] int64 and
 * log_probs [rows, num_heads] (per sub-head, not summed).
 * num_heads <= MAPPO_MULTI_SAMPLE_MAX_HEADS, every head_sizes[k] >= 1, sum of head_sizes <= 64. */
int mappo_multi_categorical_mode(const float* logits, const int* head_sizes, int num_heads, int64_t* actions,
                                 float* log_probs, int64_t rows, mappo_stream_t stream);

/* --------------------------------------------------------------- K8: GRU cell gates ----
 * Everything of one GRU step that is not a GEMM (reference onpolicy/algorithms/utils/rnn.py:7-80 runs
 * nn.GRU; PyTorch cell, gates stacked r|z|n), reading / writing the per-sequence buffers in place:
 *   r = sigmoid(gi_r + b_ir + gh_r + b_hr), z = sigmoid(gi_z + b_iz + gh_z + b_hz),
 *   n = tanh(gi_n + b_in + r * (gh_n + b_hn)), h' = n + z * (hm - n)
 * mappo_gru_cell_fwd: gi, gh [B, 3H] (input / hidden projections without bias), hm [B, H] (previous state,
 *   already multiplied by this step's mask), b_ih, b_hh [3H]; writes h_out [B, H] = h', optionally
 *   hm_next [B, H] = h' * mask_next[row] (mask_next [B]: the next step's episode-boundary mask, rnn.py:43-77;
 *   NULL mask = 1) and ws [B, 4H] = {r, z, n, gh_n + b_hn} for the backward.
 * mappo_gru_cell_bwd: g = dout + carry * mask_next (dout [B, H] = d loss / d h' from the layers above, carry
 *   [B, H] = d loss / d hm of the next step, either may be NULL); writes dgi, dgh [B, 3H] (gradients of the
 *   two projections; their column sums are the bias gradients) and dhx [B, H] = g * z, the direct part of
 *   d loss / d hm (the caller adds dgh W_hh). */
int mappo_gru_cell_fwd(const float* gi, const float* gh, const float* hm, const float* b_ih, const float* b_hh,
                       const float* mask_next, float* h_out, float* hm_next, float* ws, int64_t B, int H,
                       mappo_stream_t stream);
int mappo_gru_cell_bwd(const float* dout, const float* carry, const float* mask_next, const float* ws,
                       const float* hm, float* dgi, float* dgh, float* dhx, int64_t B, int H,
                       mappo_stream_t stream);

/* mappo_gru_step_fwd: a whole forward GRU step for H = 64 (MAPPO_E_SHAPE otherwise) -- the hidden projection
 * hm W_hh^T runs on the f32 MFMA inside the kernel with W_hh [3H, H] held in LDS, so the [B, 3H] projection
 * never goes through HBM and no separate skinny GEMM is launched.  Same buffers and semantics as
 * mappo_gru_cell_fwd without `gh`. */
int mappo_gru_step_fwd(const float* gi, const float* hm, const float* w_hh, const float* b_ih, const float* b_hh,
                       const float* mask_next, float* h_out, float* hm_next, float* ws, int64_t B, int H,
                       mappo_stream_t stream);

/* --------------------------------------------------------------- K12: the GRU over a whole chunk ----
 * RNNLayer of the recurrent policies (reference onpolicy/algorithms/utils/rnn.py:7-80: nn.GRU, gates r | z | n, state
 * multiplied by the episode mask before every step, LayerNorm on the outputs) for H = 64, ONE launch per direction over
 * the [L * mb, 64] chunk rows of recurrent_generator (shared_buffer.py:499-608; row l * mb + j = step l of chunk j; the
 * rollout is the case L = 1).  A wave walks the L steps of 32 chunks with the state in registers; both projections of a
 * step run on the matrix cores against weights held in LDS (field `arith`: MAPPO_ARITH_SIX_TERM = bf16 planes of the weights in
 * LDS, the step's input and state split once and reused by the three gates, all six blocks of the backward's transposed products
 * as planes; MAPPO_ARITH_F32_MFMA = float32 operands); gates, mask reset and the output LayerNorm on the accumulators.
 * mappo_gru_seq_forward: x, h0 [mb, 64], masks [L * mb] -> y = LayerNorm(h_l) [L * mb, 64], h_last [mb, 64] (optional).
 *   For the backward (all three or none): gates [mappo_gru_seq_gates_floats(L, mb)] (r, z, n, W_hn hm + b_hn and the
 *   normalised output per row and step, opaque order), hm [L * mb, 64] (the masked previous state of every step),
 *   stats [mappo_gru_seq_stats_floats(L, mb)].
 * mappo_gru_seq_backward (truncated BPTT inside the launch): dy [L * mb, 64] (+ dh_last [mb, 64], optional) -> dx [L * mb, 64], dh0 [mb, 64] (optional),
 *   dgi [L * mb, 192] = gradient at W_ih x + b_ih, dq [L * mb, 64] = gradient at W_hn hm + b_hn (the r and z thirds of the
 *   hidden side's gradient are dgi's) -- the caller forms dW_ih = dgi^T x and dW_hh = [dgi_rz | dq]^T hm from them -- and
 *   ln_grads [800] = LayerNorm weight | bias gradients [128], then the column sums of dgi [192] (= db_ih; its first 128 are
 *   also the r and z thirds of db_hh) and of dq [64] (= the n third of db_hh), folded over the rows inside the launch
 *   (then, with a head of <= 6 outputs, its sums: see head_w below);
 *   workspace [mappo_gru_seq_workspace_floats()] scratch.  Deterministic run to run. */
typedef struct mappo_gru_seq {
    const float* x;
    const float* h0;
    const float* masks;
    const float* w_ih;      /* [192, 64] */
    const float* w_hh;      /* [192, 64] */
    const float* b_ih;      /* [192] */
    const float* b_hh;      /* [192] */
    const float* ln_g;      /* [64] */
    const float* ln_b;      /* [64] */
    float ln_eps;
    int32_t H;              /* 64 */
    int32_t L;
    int32_t arith;          /* MAPPO_ARITH_* (occupies what was padding in ABI version 1: the layout is unchanged) */
    int64_t mb;
    float* y;
    float* h_last;
    float* gates;
    float* hm;
    float* stats;
    const float* dy;
    float* dx;
    float* dgi;
    float* dq;
    float* dh0;
    const float* dh_last;   /* [mb, 64] gradient at h_last, or NULL */
    float* ln_grads;        /* [800], see above */
    float* workspace;
    /* Optional output Linear on y inside the launches (the Categorical head's Linear, distributions.py:55-68, or the
     * critic's v_out, r_actor_critic.py:147-175): head_out > 0 makes the forward also write logits [L * mb, head_out] =
     * y head_w^T + head_b (y may then be NULL), and the backward (head_out <= 18) form dy = dlogits head_w itself from
     * dlogits [L * mb, head_out] -- dy is not read.  The head's own gradients: with head_sums = 1 (head_out <= 6) the backward also leaves
     * ln_grads[384 + 64 o + f] = sum over rows of dlogits[o] n^[f] (n^ = the normalised output, y = n^ ln_g + ln_b) and
     * ln_grads[768 + o] = sum of dlogits[o], from which dW_h = ln_g (.) GH + ln_b (x) db_h, db_h = the second sums -- y is
     * never needed; wider heads: dlogits^T y and the column sums of dlogits, formed by the caller from y. */
    const float* head_w;    /* [head_out, 64] or NULL */
    const float* head_b;    /* [head_out] */
    int32_t head_out;       /* 0: no head */
    float* logits;
    const float* dlogits;
    int32_t head_sums;      /* backward: 1 = leave the head's gradient sums in ln_grads (head_out <= 6) */
} mappo_gru_seq_t;
int64_t mappo_gru_seq_gates_floats(int L, int64_t mb);
int64_t mappo_gru_seq_stats_floats(int L, int64_t mb);
int64_t mappo_gru_seq_workspace_floats(void);
int     mappo_gru_seq_forward(const mappo_gru_seq_t* seq, mappo_stream_t stream);
int     mappo_gru_seq_backward(const mappo_gru_seq_t* seq, mappo_stream_t stream);
/* The weight gradients of that GRU from what mappo_gru_seq_backward left (reference: autograd through nn.GRU,
 * onpolicy/algorithms/utils/rnn.py:24-80), ONE launch + a reduction, float32 products from six bf16 x bf16 terms
 * (MAPPO_ARITH_SIX_TERM; the float32-MFMA route forms them with library GEMMs on the host side):
 *   dw[0 .. 192 * 64)          = dW_ih = dgi^T x                      dgi [rows, 192], x [rows, 64] (the GRU's inputs)
 *   dw[192 * 64 .. 2 * 192 * 64) = dW_hh = [dgi_r | dgi_z | dq]^T hm    dq [rows, 64], hm [rows, 64] (mask * h_{t-1})
 * rows = L * mb; all pointers 16-byte aligned; workspace [mappo_gru_weight_grads_workspace_floats()] scratch.  Deterministic. */
int64_t mappo_gru_weight_grads_workspace_floats(void);
int     mappo_gru_weight_grads(const float* dgi, const float* dq, const float* x, const float* hm, int64_t rows, float* dw,
                               float* workspace, mappo_stream_t stream);

/* --------------------------------------------------------------- K13: gradient clipping + Adam of one network ----
 * What the reference does between backward() and the next minibatch for each network (r_mappo.py:146-167:
 * nn.utils.clip_grad_norm_(parameters, max_grad_norm) or get_gard_norm, then optimizer.step(); the optimiser is
 * torch.optim.Adam(lr, eps = opti_eps, weight_decay), rMAPPOPolicy.py:31-37) as two launches over all tensors of the
 * network: total L2 norm of the gradients -> grad_norm [1] (before clipping), gradients scaled in place by
 * min(1, max_grad_norm / (norm + 1e-6)) (max_grad_norm <= 0: no clipping), then Adam without amsgrad on the optimiser's
 * own state tensors: step[t] (float32 scalar, incremented), exp_avg[t], exp_avg_sq[t], param[t], all float32 and
 * contiguous.  workspace [mappo_adam_workspace_floats()]. */
#define MAPPO_ADAM_MAX_TENSORS 64
typedef struct mappo_adam {
    float*  param[MAPPO_ADAM_MAX_TENSORS];
    float*  grad[MAPPO_ADAM_MAX_TENSORS];
    float*  exp_avg[MAPPO_ADAM_MAX_TENSORS];
    float*  exp_avg_sq[MAPPO_ADAM_MAX_TENSORS];
    float*  step[MAPPO_ADAM_MAX_TENSORS];
    int64_t numel[MAPPO_ADAM_MAX_TENSORS];
    int32_t n;
    double  lr, beta1, beta2, eps, weight_decay, max_grad_norm;     /* doubles, as torch.optim.Adam holds them */
    float*  grad_norm;
    float*  workspace;
    const double* lr_device;    /* optional: the learning rate is read from this device double instead of `lr` -- a launch that
                                   was captured into a HIP graph then follows lr_decay (rMAPPOPolicy.py:39-46) between replays */
} mappo_adam_t;
int64_t mappo_adam_workspace_floats(void);
int     mappo_clip_adam(const mappo_adam_t* adam, mappo_stream_t stream);

/* ValueNorm.update + running_mean_var as two launches (reference onpolicy/utils/valuenorm.py:32-55): the mean and mean of
 * squares of x [n] (or batch_moments [2] = {mean, mean_sq} when the caller all-reduced them over the ranks; x is then
 * ignored) are folded into the scalar statistics in place, m <- weight * m + (1 - weight) * E[.], debiasing_term <-
 * weight * d + (1 - weight), and denorm [2] receives {sigma, mu} = {sqrt(max(m2 / max(d, eps) - mu^2, 1e-2)), m1 / max(d,
 * eps)} -- what the loss normalises returns with and the GAE scan de-normalises values with.
 * workspace [mappo_valuenorm_workspace_doubles()] float64. */
int64_t mappo_valuenorm_workspace_doubles(void);
int     mappo_valuenorm_update(const float* x, int64_t n, const float* batch_moments, double weight, float eps,
                               float* running_mean, float* running_mean_sq, float* debiasing_term, float* denorm,
                               double* workspace, mappo_stream_t stream);

/* What a minibatch needs before its loss is formed (reference onpolicy/algorithms/r_mappo/r_mappo.py:135-139 and :84-87: the
 * masked means divide by active_masks.sum(), the unmasked ones by the row count; :65 feeds ValueNorm / PopArt with the batch
 * moments of the returns), three launches instead of ~13 PyTorch ones (27 with the data-parallel bookkeeping).
 * mappo_minibatch_sums: active_masks [n], returns [n] -> sums [4] float64 = {sum active_masks, n, sum returns,
 *   sum returns^2} (fixed summation order).  A data-parallel caller all-reduces a copy of them over the ranks.
 * mappo_minibatch_scales: local / global sums (the same array for one rank) -> out [8] float32 =
 *   {1 / global policy denominator, 1 / global value denominator, 1 / local policy denominator (twice), 1 / local value
 *   denominator, 1 / local rows, mean and mean of squares of the returns over the global minibatch}; a denominator is the
 *   active-mask sum when the loss is masked (use_policy_active_masks / use_value_active_masks), else the row count.
 *   out[0..1] scale the fused loss (K7: `inv`), out[2..5] turn its four sums into the logged means, out[6..7] are
 *   mappo_valuenorm_update's batch_moments. */
int64_t mappo_minibatch_sums_workspace_doubles(void);
int     mappo_minibatch_sums(const float* active_masks, const float* returns, int64_t n, double* sums, double* workspace,
                             mappo_stream_t stream);
int     mappo_minibatch_scales(const double* local_sums, const double* global_sums, int policy_masked, int value_masked,
                               float* out, mappo_stream_t stream);

/* --------------------------------------------------------------- K10: sort-free minibatch index lists ----
 * Device-side replacement of `rand = torch.randperm(B); slices = [rand[i*mb:(i+1)*mb] for i in range(n_mb)]`
 * (reference onpolicy/utils/shared_buffer.py:360-361 feed-forward, :415-416 whole trajectories, :511-512 chunks).
 * Sample r belongs to slice perm(r) / mb, perm = a keyed bijection of [0, n) (6-round balanced Feistel network with
 * cycle walking, keys[0..5] = 32-bit round keys drawn by the caller); samples with perm(r) >= n_mb * mb are dropped,
 * as the reference drops the permutation's tail.  idx [n_mb * mb] int64 receives the slices back to back, every
 * slice in ASCENDING sample order (a minibatch is a set: its loss does not depend on row order, and ascending order turns
 * the gathers into monotonic walks over the buffer).  No sort, no n-sized temporary: workspace
 * [mappo_minibatch_workspace_ints(n, n_mb)] int32.  n_mb <= MAPPO_PERM_MAX_MINIBATCHES.  The integer-parity mode of the
 * samplers (--sampler_rng host) does not use this: it uploads the reference's CPU permutation unchanged. */
#define MAPPO_PERM_MAX_MINIBATCHES 64
int64_t mappo_minibatch_workspace_ints(int64_t n, int n_mb);
int     mappo_minibatch_indices(int64_t n, int64_t mb, int n_mb, const uint32_t* keys, int64_t* idx, int32_t* workspace,
                                mappo_stream_t stream);

/* --------------------------------------------------------------- K9: fused hidden-64 trunk ----
 * The actor / critic network of the update as three kernels instead of ~25 launches per minibatch span: what
 * MLPBase + the output Linear compute (reference onpolicy/algorithms/utils/mlp.py:6-58: [LayerNorm(obs)] ->
 * (Linear -> Tanh | ReLU -> LayerNorm) x (1 + layer_N); act.py / distributions.py:55-68 Categorical head and
 * r_actor_critic.py:147-175 v_out are plain Linears on the trunk's features), evaluated straight from the rollout
 * buffer: the rows are read through the sampler's index list (shared_buffer.py:379-396 rows mode, :554-604 chunk
 * mode), so the gathered [mb, obs_dim] minibatch of feed_forward_generator / recurrent_generator is never written.
 * hidden_size must be 64.  The matrix products run in the arithmetic the call's `arith` field names (MAPPO_ARITH_* above).
 *
 * Rows: the caller resolves the sampler's row map once per minibatch into a row table (mappo_mlp_row_table): the source
 * row (int32) of every launch row, mappo_mlp_row_table_ints(rows) = rows rounded up to 128 entries (padding entries repeat
 * the last row, so no kernel clamps a row index).  The kernels then issue coalesced table loads instead of a dependent
 * idx chain and do no index arithmetic.  Input LayerNorm: pass src = a standardised copy of the observation matrix
 * (mappo_standardize_rows, made once per train() -- the observations do not change during the ppo epochs) and fold the
 * LayerNorm's affine half into the first Linear on the caller's side (w1 = W * gamma, bias[0] = b + W beta); the kernels
 * themselves use the rows as they are (use_feature_normalization = False: src = the field itself).
 *
 *   src        [src_rows, din]   matrix the rows come from (e.g. buffer.share_obs[:-1] viewed [T*N*A, din])
 *   row_tab    see above (int32, 16-byte aligned); din >= 4
 *   w1 [64, din], bias[l] / ln_g[l] / ln_b[l] [64] for l < n_layers (n_layers = 1 + layer_N <= 3), w2[l-1] [64, 64]
 *   act        1 Tanh, 2 ReLU (0 identity)
 *   wh [out, 64], bh [out]   output Linear (out <= 64); out = 0: y receives the trunk's features [rows, 64]
 * mappo_mlp_forward writes y [rows, out] and, when z[l] != NULL, what the backward needs of every layer: z[l] = the
 *   LayerNorm's normalised input (act(.) - mean) * rstd, 64 floats for each of mappo_mlp_row_table_ints(rows) rows (rows
 *   rounded up to 128) in the kernels' own order -- opaque scratch between the two calls: element (row r, feature
 *   32 t + 8 q + 4 h + e) sits at float (r / 32) * 2048 + (4 t + q) * 256 + (32 h + r % 32) * 4 + e -- and ln_stats[l]
 *   = {mean, rstd} per row, room for the same padded row count (both NULL in rollouts).
 * mappo_mlp_backward reads dy [rows, out] (or [rows, 64] for out = 0), z[l] and ln_stats[l]; writes `grads`, the parameter gradients
 *   as one flat array [w1 64*din | per layer: bias 64, ln weight 64, ln bias 64 | per hidden layer: w 64*64 | wh out*64 |
 *   bh out] (mappo_mlp_grad_floats), using dz1 [mappo_mlp_row_table_ints(rows), 64] and workspace [mappo_mlp_workspace_floats] as scratch.
 *   Gradients are plain sums over the rows in a fixed order (deterministic run to run).
 * mappo_mlp_row_table: idx [mb] int64 sampler indices (NULL: launch row r = source row r);
 *   chunk_len 0: rows mode (rows = mb, row r <- idx[r]); L > 0: chunk mode, rows = L * mb, row l * mb + j <- element
 *   idx[j] * L + l of the (n, a, t)-ordered sequence (needs T, N, A). */
#define MAPPO_MLP_MAX_LAYERS 3
typedef struct mappo_mlp {
    const float* src;
    const int32_t* row_tab;
    int64_t rows;
    int32_t din, n_layers, act, out;
    float ln_eps;
    int32_t arith;      /* MAPPO_ARITH_* (occupies what was padding in ABI version 1: the layout is unchanged) */
    const float* w1;
    const float* bias[MAPPO_MLP_MAX_LAYERS];
    const float* ln_g[MAPPO_MLP_MAX_LAYERS];
    const float* ln_b[MAPPO_MLP_MAX_LAYERS];
    const float* w2[MAPPO_MLP_MAX_LAYERS - 1];
    const float* wh;
    const float* bh;
    float* y;
    float* z[MAPPO_MLP_MAX_LAYERS];
    float* ln_stats[MAPPO_MLP_MAX_LAYERS];
    const float* dy;
    float* dz1;
    float* workspace;
    float* grads;
} mappo_mlp_t;
int64_t mappo_mlp_row_table_ints(int64_t rows);
int     mappo_mlp_row_table(const int64_t* idx, int64_t rows, int64_t mb, int chunk_len, int T, int N, int A,
                            int32_t* row_tab, mappo_stream_t stream);
/* tuning / test hook: at most `cap` workgroups per K9 kernel (0 = default sizing); small caps make every workgroup loop
 * over many tiles */
int     mappo_mlp_set_grid_cap(int cap);
/* tuning hook: device buffer of >= 512 int64 that receives shader-clock stamps of workgroup 0's first pipeline
 * iterations of mappo_mlp_forward (tools/bench_mlp.py --stamps), NULL = off */
int     mappo_mlp_set_debug(long long* buf);
/* tuning / test hook: option bits of the K9 launchers (initial value: environment variable MAPPO_MLP_FLAGS, default 0);
 * returns the previous value, or -1 (nothing changed) for a bit that does not exist.  NONE of them selects arithmetic
 * (that is the per-call `arith` field).  1 = the forward's compute waves keep the default priority; 2 = K15's forward
 * (mappo_linear512_forward) issues its MFMAs in four groups of four feature tiles per step (round 5's form; default: eight
 * groups of two); 8 = K15's weight gradient (mappo_linear512_wgrad): every wave reads and splits all four column tiles of X
 * itself (round 5's form; default: one tile per wave, shared through LDS as bf16 planes); 4 = mappo_mlp_forward
 * keeps the loader / compute kernel (mlp_fwd_kernel) for shapes the version-3 kernel (operands straight from global memory,
 * resident first-layer weights; aligned rows up to 448 floats wide, two or three layers) would take; 32 = the OTHER form of
 * the direct-to-LDS first-layer weight-gradient kernel: under MAPPO_ARITH_F32_MFMA two slots per wave and two workgroups per
 * CU (default: four slots, one workgroup), under MAPPO_ARITH_SIX_TERM four slots and one workgroup (default: two and two);
 * 128 = under MAPPO_ARITH_SIX_TERM the version-4 forward (first layer in six-term form, one wave per SIMD) also for aligned inputs narrower than 128 floats,
 * which by default take version 3 with only the hidden layer in six-term form (tests: every chunk shape of version 4);
 * 256 = under MAPPO_ARITH_SIX_TERM two-layer trunks with aligned inputs of at most 64 columns keep the separate first-layer
 * weight-gradient kernel (mlp_dw1_rows_kernel) instead of accumulating that gradient inside the chain's launch (A/B, tests);
 * 16384 = under MAPPO_ARITH_SIX_TERM the two-slot direct first-layer weight-gradient kernel of inputs up to 384 floats wide
 * lets every wave split the whole dz1 tile into bf16 planes itself (default: once per workgroup, every wave its own four rows,
 * the planes shared through LDS); the same bits either way (A/B, tests). */
int     mappo_mlp_set_flags(int flags);
int     mappo_mlp_forward(const mappo_mlp_t* net, mappo_stream_t stream);
int     mappo_mlp_backward(const mappo_mlp_t* net, mappo_stream_t stream);
int64_t mappo_mlp_grad_floats(int din, int n_layers, int out);
int64_t mappo_mlp_workspace_floats(int din, int n_layers, int out);
/* dst[r, :] = (src[r, :] - mean_r) / sqrt(var_r + eps) for every row of a [rows, D] matrix (population variance: the
 * parameter-free half of nn.LayerNorm, reference onpolicy/algorithms/utils/mlp.py:47-48, 56-57) */
int     mappo_standardize_rows(const float* src, int64_t rows, int D, float eps, float* dst, mappo_stream_t stream);
/* ... with the rows of dst `ld` >= D floats apart and zeros in columns D .. ld - 1: a copy padded to a multiple of 4
 * floats lets the trunk kernels take their 16-byte aligned paths for odd observation widths (pass din = ld and a
 * first-layer weight matrix padded with zero columns; the zero products change no bit of the result) */
int     mappo_standardize_rows_ld(const float* src, int64_t rows, int D, float eps, float* dst, int ld,
                                  mappo_stream_t stream);
/* The affine half of that LayerNorm folded into the Linear behind it (reference mlp.py:47-48 feature_norm, :20 fc1):
 * Linear(LayerNorm(x)) = x^ w_folded^T + b_folded with w_folded[f][k] = w[f][k] gamma[k] (rows `ld` >= din floats apart,
 * zero columns beyond din: the padded copy above), b_folded[f] = b[f] + sum_k w[f][k] beta[k].  One launch; the
 * backward turns the gradients at (w_folded [out_features, ld], b_folded) into those of w [out_features, din], gamma,
 * beta [din] (the gradient of b is db_folded itself), one launch. */
int     mappo_fold_input_norm_forward(const float* w, const float* b, const float* gamma, const float* beta, int out_features,
                                      int din, int ld, float* w_folded, float* b_folded, mappo_stream_t stream);
int     mappo_fold_input_norm_backward(const float* w, const float* gamma, const float* beta, const float* dw_folded,
                                       const float* db_folded, int out_features, int din, int ld, float* dw, float* dgamma,
                                       float* dbeta, mappo_stream_t stream);

/* --------------------------------------------------------------- K15: tall Linear layers with 512 outputs ----
 * The GEMMs of the hidden-512 trunks (BASELINE configs[4], Hanabi: reference onpolicy/algorithms/utils/mlp.py:6-58 at
 * --hidden_size 512 --layer_N 2, scripts/train_hanabi_forward.sh:15-17) in MAPPO_ARITH_SIX_TERM arithmetic: float32 in,
 * float32 out, every product from six bf16 x bf16 terms of the operands' exact three-way splits on the bf16 matrix cores,
 * float32 accumulation.  (Callers that want the float32 matrix instruction use the library GEMM: torch.nn.functional.linear.)
 *   mappo_linear512_prepare:  the three bf16 planes of W [512, K] (rows ldw floats apart) -- or, transposed = 1, of W^T for a
 *     W whose element (k, feature) is w[k * ldw + feature] (the input gradient of a 512 -> 512 Linear: dX = dY W) -- in the
 *     order the forward reads them; planes [mappo_linear512_planes_floats(K)] floats, 16-byte aligned.  Once per weight value.
 *   mappo_linear512_forward:  y [rows, 512] = x [rows, K] W^T (+ bias [512] unless NULL); x rows ldx >= K floats apart
 *     (columns K .. ldx - 1 must hold finite values: the zero padding of mappo_standardize_rows_ld); rows that start on 16-byte
 *     boundaries (ldx a multiple of 4) are loaded in 16-byte pieces, any other ldx (Hanabi's 1285 / 1385-wide gathered
 *     minibatches) in 4-byte pieces.  planes, y and bias must be 16-byte aligned (MAPPO_E_ALIGN otherwise).
 *   mappo_linear512_forward_norm:  a whole block Sequential(Linear, ReLU, LayerNorm) of the reference's MLPLayer (mlp.py:17-22)
 *     in the forward's launch: y [rows, 512] = x W^T + bias (the pre-activation, what mappo_bias_act_layernorm_bwd reads with
 *     a zero pre_bias), yn [rows, 512] = gamma * (relu(y) - mean) * rstd + beta, mean / rstd [rows] the statistics of
 *     relu(y) over the 512 features (biased variance, rstd = 1 / sqrt(var + eps): the arithmetic of
 *     mappo_bias_act_layernorm_fwd); act must be 2 = relu (the codes of mappo_bias_act_layernorm_fwd; MAPPO_E_FLAGS otherwise); bias, gamma, beta, planes, y,
 *     yn 16-byte aligned.  Replaces mappo_linear512_forward + mappo_bias_act_layernorm_fwd: the pre-activation is written
 *     once and not read back.
 *   mappo_linear512_wgrad:    dw [512, K] = dy^T [512, rows] x [rows, K] (the weight gradient of y = x W^T; the contraction
 *     runs over the rows, partial sums of row ranges are added in a fixed order: deterministic run to run);
 *     workspace [mappo_linear512_wgrad_workspace_floats(K)] floats. */
int64_t mappo_linear512_planes_floats(int K);
int     mappo_linear512_prepare(const float* w, int K, int ldw, int transposed, float* planes, mappo_stream_t stream);
int     mappo_linear512_forward(const float* x, int64_t rows, int K, int ldx, const float* planes, const float* bias,
                                float* y, mappo_stream_t stream);
int     mappo_linear512_forward_norm(const float* x, int64_t rows, int K, int ldx, const float* planes, const float* bias,
                                     const float* gamma, const float* beta, float eps, int act, float* y, float* yn,
                                     float* mean, float* rstd, mappo_stream_t stream);
int64_t mappo_linear512_wgrad_workspace_floats(int K);
int     mappo_linear512_wgrad(const float* dy, const float* x, int64_t rows, int K, int ldx, float* dw, float* workspace,
                              mappo_stream_t stream);

/* --------------------------------------------------------------- K11: simple_spread worlds on the device ----
 * One env step of `n_worlds` cooperative-navigation worlds (the env of BASELINE.json configs[0] / configs[2]; reference
 * onpolicy/envs/mpe/core.py:120-190, environment.py:100-180, scenarios/simple_spread.py:60-103) as one launch, so that
 * a rollout step with the policy, the env and the buffer on the GPU moves nothing over PCIe (scope row f1).  State is
 * float64 and updated in place: pos / vel [n, A, 2], landmarks [n, L, 2], t [n] int64.  actions [n, A] int64 in 0..4.
 * Worlds whose t reaches world_length report done and (auto_reset) restart from fresh_pos [n, A, 2] / fresh_landmarks
 * [n, L, 2] (uniform(-1, 1) draws for every world, used where needed).  Outputs: obs [n, A, 4 + 2 L + 4 (A - 1)]
 * float32 (of the restarted world where one restarted), rewards [n, A, 1] float32 (shared reward), dones [n, A] bytes,
 * per_agent [n, A] float64 (the individual_reward info).  A, L <= MAPPO_ENV_MAX_ENTITIES. */
#define MAPPO_ENV_MAX_ENTITIES 16
int mappo_simple_spread_step(double* pos, double* vel, double* landmarks, int64_t* t, const int64_t* actions,
                             const double* fresh_pos, const double* fresh_landmarks, float* obs, float* rewards,
                             uint8_t* dones, double* per_agent, int64_t n_worlds, int num_agents, int num_landmarks,
                             int world_length, int auto_reset, mappo_stream_t stream);

/* ----------------------------------------------------- K11 family: simple_reference worlds on the device ----
 * One env step of `n_worlds` referential-communication worlds (reference onpolicy/envs/mpe/scenarios/simple_reference.py,
 * environment.py:115-255, core.py:207-288; 2 agents, 3 landmarks, no contacts) as one launch.  State is updated in
 * place: pos / vel [n, 2, 2] and landmarks [n, 3, 2] float64, t [n] int64, goals [n, 2] int64 (each agent's goal
 * landmark, 0..2), comm [n, 2] int64 (each agent's last communication symbol, -1 = silent).  actions [n, 2, 2] int64
 * (movement 0..4, symbol 0..9).  Worlds whose t reaches world_length report done and (auto_reset) restart from
 * fresh_pos [n, 2, 2], 0.8 * fresh_landmarks [n, 3, 2] (uniform(-1, 1) draws) and fresh_goals [n, 2], with zero
 * velocity and silent agents.  Outputs: obs [n, 2, 21] float32 (velocity, landmarks relative to the agent, the
 * colour of the agent's goal landmark, the other agent's symbol one-hot; of the restarted world where one restarted),
 * rewards [n, 2, 1] float32 (shared: r_0 + r_1), dones [n, 2] bytes, per_agent [n, 2] float64 (r_i, the
 * individual_reward info). */
int mappo_simple_reference_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goals, int64_t* comm,
                                const int64_t* actions, const double* fresh_pos, const double* fresh_landmarks,
                                const int64_t* fresh_goals, float* obs, float* rewards, uint8_t* dones,
                                double* per_agent, int64_t n_worlds, int world_length, int auto_reset,
                                mappo_stream_t stream);

/* ---------------------------------------------- K11 family: simple_speaker_listener worlds on the device ----
 * One env step of `n_worlds` speaker / listener worlds (reference onpolicy/envs/mpe/scenarios/simple_speaker_listener.py
 * :38-98, environment.py:115-255, core.py:160-190 and :207-288; 2 agents, 3 landmarks, no contacts) as one launch.
 * Agent 0 (the speaker) never moves; agent 1 (the listener) is silent.  State is updated in place: pos / vel [n, 2, 2]
 * and landmarks [n, 3, 2] float64, t [n] int64, goal [n] int64 (the goal landmark, 0..2), comm [n] int64 (the speaker's
 * last symbol, -1 = silent).  actions [n, 2] int64 (the speaker's symbol 0..2, the listener's movement 0..4).  Worlds
 * whose t reaches world_length report done and (auto_reset) restart from fresh_pos [n, 2, 2], fresh_landmarks [n, 3, 2]
 * (uniform(-1, 1) draws) and fresh_goal [n], at rest and silent.  Outputs: obs [n, 14] float32, one row per world that
 * is also the centralised observation: columns 0:3 the speaker's observation (the goal landmark's colour), 3:14 the
 * listener's (velocity, landmarks relative to it, the speaker's symbol one-hot).  obs is written after a restart, so a
 * restarted world reports its fresh state; rewards, dones and per_agent are those of the step that ended the episode.
 * rewards [n, 2, 1] float32 (shared: -2 |listener - goal|^2), dones [n, 2] bytes, per_agent [n, 2] float64
 * (-|listener - goal|^2, the individual_reward info). */
int mappo_simple_speaker_listener_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goal,
                                       int64_t* comm, const int64_t* actions, const double* fresh_pos,
                                       const double* fresh_landmarks, const int64_t* fresh_goal, float* obs,
                                       float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                       int world_length, int auto_reset, mappo_stream_t stream);

/* ---------------------------------------------------------- K11 family: simple_push worlds on the device ----
 * One env step of `n_worlds` keep-away worlds (reference onpolicy/envs/mpe/scenarios/simple_push.py:41-104,
 * environment.py:115-255, core.py:160-190 and :290-321 contact forces; A = num_agents in 2..MAPPO_ENV_MAX_ENTITIES,
 * L = num_landmarks in 1..2) as one launch.  Agent 0 is the adversary, agents 1..A-1 are good; all move, are silent and
 * collide softly below distance 0.1 (coincident agents exert no force).  State is updated in place: pos / vel [n, A, 2]
 * and landmarks [n, L, 2] float64, t [n] int64, goal [n] int64 (the goal landmark all agents share, 0..L-1).  actions
 * [n, A] int64 in 0..4.  Worlds whose t reaches world_length report done and (auto_reset) restart from fresh_pos
 * [n, A, 2], 0.8 * fresh_landmarks [n, L, 2] (uniform(-1, 1) draws) and fresh_goal [n], at rest.  Outputs: obs
 * [n, Da + (A - 1) Dg] float32, one row per world that is also the centralised observation: columns 0:Da the
 * adversary's observation (velocity, landmarks and other agents relative to it; Da = 2 + 2 L + 2 (A - 1)), then Dg =
 * 7 + 5 L + 2 (A - 1) columns per good agent in agent order (velocity, the goal relative to it, its colour, landmarks
 * relative to it, the landmarks' colours, other agents relative to it).  obs is written after a restart, so a restarted
 * world reports its fresh state; rewards, dones and per_agent are those of the step that ended the episode.  The world
 * is not collaborative: rewards [n, A, 1] float32 and per_agent [n, A] float64 (the individual_reward info) both hold
 * each agent's own reward, -|pos - goal| for a good agent and min over good agents |pos_g - goal| - |pos - goal| for the
 * adversary; dones [n, A] bytes.  MAPPO_E_SHAPE for A < 2 or L outside 1..2, MAPPO_E_TOO_MANY for A > 16. */
int mappo_simple_push_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* goal,
                           const int64_t* actions, const double* fresh_pos, const double* fresh_landmarks,
                           const int64_t* fresh_goal, float* obs, float* rewards, uint8_t* dones, double* per_agent,
                           int64_t n_worlds, int num_agents, int num_landmarks, int world_length, int auto_reset,
                           mappo_stream_t stream);

/* ----------------------------------------------------------- K11 family: simple_tag worlds on the device ----
 * One env step of `n_worlds` predator-prey worlds (reference onpolicy/envs/mpe/scenarios/simple_tag.py:6-144,
 * environment.py:115-255, core.py:207-321: action force, integration with a top speed, contact forces; A = num_agents in
 * 2..MAPPO_ENV_MAX_ENTITIES, Nadv = num_adversaries in 1..A-1, L = num_landmarks in 1..MAPPO_TAG_MAX_LANDMARKS) as one
 * launch.  Agents 0..Nadv-1 are adversaries (radius 0.075, acceleration 3, top speed 1.0), the G = A - Nadv agents after
 * them are good (0.05, 4, 1.3); all move, are silent and collide softly with each other below the sum of their radii and
 * with the landmarks (radius 0.2, immovable: the agent alone takes the force) below radius + 0.2; coincident centres
 * exert no force.  The action force is acceleration^2 times the direction, 9 or 16 (the reference applies the
 * acceleration as the action's sensitivity and as the force's factor); after damping and force the speed is clamped to
 * the top speed.  State is updated in place: pos / vel [n, A, 2] and landmarks [n, L, 2] float64, t [n] int64.  actions
 * [n, A] int64 in 0..4.  Worlds whose t reaches world_length report done and (auto_reset) restart from fresh_pos
 * [n, A, 2] and 0.8 * fresh_landmarks [n, L, 2] (uniform(-1, 1) draws), at rest.  Outputs: obs [n, Nadv Da + G Dg]
 * float32, one row per world that is also the centralised observation, the agents' columns in agent order: velocity,
 * position, landmarks relative to the agent, other agents relative to it, the velocities of the other good agents
 * (Da = 4 + 2 L + 2 (A - 1) + 2 G for an adversary, Dg = Da - 2 for a good agent).  obs is written after a restart, so a
 * restarted world reports its fresh state; rewards, dones and per_agent are those of the step that ended the episode.
 * The world is not collaborative: rewards [n, A, 1] float32 and per_agent [n, A] float64 (the individual_reward info)
 * both hold each agent's own reward.  With hits the number of (good agent, adversary) pairs closer than 0.125, every
 * adversary is paid 10 hits; a good agent -10 per adversary closer to it than 0.125, minus bound(|x|) + bound(|y|) with
 * bound(x) = 0 below 0.9, 10 (x - 0.9) below 1.0 and min(exp(2 x - 2), 10) from there on; dones [n, A] bytes.
 * MAPPO_E_SHAPE for Nadv outside 1..A-1 or L < 1, MAPPO_E_TOO_MANY for A > 16 or L > 4. */
#define MAPPO_TAG_MAX_LANDMARKS 4
int mappo_simple_tag_step(double* pos, double* vel, double* landmarks, int64_t* t, const int64_t* actions,
                          const double* fresh_pos, const double* fresh_landmarks, float* obs, float* rewards,
                          uint8_t* dones, double* per_agent, int64_t n_worlds, int num_agents, int num_adversaries,
                          int num_landmarks, int world_length, int auto_reset, mappo_stream_t stream);

/* ---------------------------------------------------- K11 family: simple_world_comm worlds on the device ----
 * One env step of `n_worlds` worlds of predator-prey with forests, food and a speaking leader (reference
 * onpolicy/envs/mpe/scenarios/simple_world_comm.py, environment.py:54-98 and :115-255, core.py:207-321; A = num_agents in
 * 2..MAPPO_ENV_MAX_ENTITIES, Nadv = num_adversaries in 1..A-1, L = num_landmarks, the obstacles, in
 * 1..MAPPO_WORLD_COMM_MAX_OBSTACLES) as one launch.  Agents, forces, top speeds and integration are simple_tag's with a
 * good agent's radius 0.045.  The landmark list holds L obstacles (radius 0.2, the only ones that exert contact forces),
 * then 2 pieces of food (0.03), then 2 forests (0.3): Lt = L + 4.  Agent 0, the leader, also says a word.  State is
 * updated in place: pos / vel [n, A, 2] and landmarks [n, Lt, 2] float64, t [n] and comm [n] int64 (the leader's last
 * word, -1 while nothing has been said since a restart).  actions [n, A + 1] int64: the leader's movement 0..4, its word
 * 0..3, the other agents' movements.  Worlds whose t reaches world_length report done and (auto_reset) restart from
 * fresh_pos [n, A, 2] and 0.8 * fresh_landmarks [n, Lt, 2] (uniform(-1, 1) draws), at rest, comm -1.
 * Agent i is inside forest f when closer to its centre than its radius + 0.3, and sees agent j iff i is the leader, both
 * are inside forest 0, both are inside forest 1, or neither is inside any forest.  Outputs: obs [n, Nadv Da + G Dg]
 * float32, one row per world that is also the centralised observation, the agents' columns in agent order.  An
 * adversary: velocity, position, landmarks relative to the agent, other agents relative to it ((0, 0) for one it does
 * not see), the good agents' velocities ((0, 0) likewise), inside forest 0 / 1 as +-1, comm as a one-hot of 4
 * (Da = 4 + 2 Lt + 2 (A - 1) + 2 G + 6).  A good agent: velocity, position, landmarks, other agents (masked), the two
 * forest flags, the other good agents' velocities (masked) (Dg = 4 + 2 Lt + 2 (A - 1) + 2 + 2 (G - 1)).  obs is written
 * after a restart, so a restarted world reports its fresh state; rewards, dones and per_agent are those of the step that
 * ended the episode.  The world is not collaborative: rewards [n, A, 1] float32 and per_agent [n, A] float64 both hold
 * each agent's own reward.  With hits the number of (good agent, adversary) pairs closer than 0.12, adversary a is paid
 * 5 hits - 0.1 x its distance to the nearest good agent; a good agent -5 per adversary closer to it than 0.12,
 * -2 (bound(|x|) + bound(|y|)) with simple_tag's bound, +2 per food closer than 0.075 and +0.05 x its distance to the
 * nearest food; dones [n, A] bytes.  MAPPO_E_SHAPE for Nadv outside 1..A-1 or L < 1, MAPPO_E_TOO_MANY for A > 16 or
 * L > 4. */
#define MAPPO_WORLD_COMM_MAX_OBSTACLES 4
int mappo_simple_world_comm_step(double* pos, double* vel, double* landmarks, int64_t* t, int64_t* comm,
                                 const int64_t* actions, const double* fresh_pos, const double* fresh_landmarks,
                                 float* obs, float* rewards, uint8_t* dones, double* per_agent, int64_t n_worlds,
                                 int num_agents, int num_adversaries, int num_landmarks, int world_length,
                                 int auto_reset, mappo_stream_t stream);

/* ------------------------------------------------------------------- K16: Hanabi tables on the device ----
 * The batched Hanabi stepper of include/hanabi_batch.h (libhanabi_batch.so, host) with its tables in device memory: the
 * same rules, deal and encoder source (csrc/hanabi_rules.h), so for equal seeds and moves every row, reward, status and
 * score equals the host stepper's -- and through it the reference engine's -- bit for bit.  What it replaces in the
 * reference (marlbenchmark/on-policy) is what include/hanabi_batch.h lists: hanabi_lib/hanabi_state.cc:84-96, :164-283,
 * :327-339, :364-382; hanabi_game.cc:50, :108-114, :162-196; canonical_encoders.cc:64-115, :133-182, :204-230, :259-342,
 * :377-433, :482-536, :575-594; the per-env glue onpolicy/envs/hanabi/Hanabi_Env.py:278-312 (reset), :451-500 (step).
 *
 * The rule set is passed BY VALUE as the eight int32 fields of hanabi_rules_t in its order (colors, ranks, players,
 * hand_size, max_information_tokens, max_life_tokens, observation_type, random_start_player), with its limits (5 colours,
 * 5 ranks, 5 players, 5 cards a hand; tokens <= 1024).  random_start_player != 0 is MAPPO_E_SHAPE: that draw is a
 * std::uniform_int_distribution, whose algorithm differs between library versions.  A rule set whose row image
 * (observation | centralised row | legal moves) exceeds 48 KiB is MAPPO_E_SHAPE too.  share_mode: enum hanabi_share_mode.
 *
 * State is caller-owned: n_tables * mappo_hanabi_state_bytes(rules) bytes, 4-byte aligned, laid out by the library as
 * the generators' words [624][n_tables] uint32 (word k of table n at k * n_tables + n: the tables of a wave touch
 * neighbouring words) followed by n_tables game records (~240 bytes each, array of structs).  The library allocates
 * nothing.  Row arrays are [n_tables, width] float32, 16-byte aligned (else MAPPO_E_ALIGN):
 *   obs        width obs_len + players                  observation | one-hot turn of the player to move
 *   share_obs  width own_hand_len + obs_len + players   (HANABI_SHARE_OWN_HAND) or players * obs_len + players
 *   available  width num_moves                          1 where the move uid is legal
 * to_move [n] int32 (may be NULL): the player to move, -1 for zero rows.
 * flags [n] int32, the one word per table a host needs to drive the turn-based runner:
 *   bits 0-7 status (0 running, 1 finished, 2 idle, 255 refused), bit 8 "some move is legal", bits 16-31 the score.
 * Argument errors (MAPPO_E_NULL / _SHAPE / _ALIGN) are returned before anything touches the device. */

/* Bytes of table state per table (negative: MAPPO_E_SHAPE for a rule set outside the limits). */
int64_t mappo_hanabi_state_bytes(int32_t colors, int32_t ranks, int32_t players, int32_t hand_size,
                                 int32_t max_information_tokens, int32_t max_life_tokens, int32_t observation_type,
                                 int32_t random_start_player);
/* dims[5] (HOST pointer) = players, num_moves (HanabiGame::MaxMoves), obs_len, own_hand_len, hand_size in force. */
int mappo_hanabi_dims(int32_t colors, int32_t ranks, int32_t players, int32_t hand_size, int32_t max_information_tokens,
                      int32_t max_life_tokens, int32_t observation_type, int32_t random_start_player, int32_t* dims);

/* One generator per table from seeds[n] (device, int32 taken modulo 2^32) exactly as std::mt19937::seed does
 * (hanabi_game.cc:50): s[0] = seed, s[k] = 1812433253 (s[k-1] ^ s[k-1] >> 30) + k, next word 624; the table is marked
 * as not started and its draw counter is zeroed.  The generator keeps running across the games of its table. */
int mappo_hanabi_seed(void* state, const int32_t* seeds, int64_t n_tables, mappo_stream_t stream);

/* hanabi_batch_reset(choose) + hanabi_batch_encode(choose) (Hanabi_Env.py:278-312): a new game on every table with
 * choose[n] != 0 (device uint8), dealt until a player is to move (hanabi_state.cc:327-339: discrete distribution over the
 * card types in stock, written out -- weights stock / total in card order, normalised, running sums with the last set to
 * 1, p from two generator words (low first) as a double in [0, 1), the first running sum >= p; one type left: no word
 * is drawn), then its rows.  Tables not chosen keep their game and get zero rows, to_move -1, status 2.  Two launches. */
int mappo_hanabi_reset(void* state, const uint8_t* choose, float* obs, float* share_obs, float* available,
                       int32_t* to_move, int32_t* flags, int64_t n_tables, int share_mode, int32_t colors,
                       int32_t ranks, int32_t players, int32_t hand_size, int32_t max_information_tokens,
                       int32_t max_life_tokens, int32_t observation_type, int32_t random_start_player,
                       mappo_stream_t stream);

/* hanabi_batch_step + hanabi_batch_encode(actions != -1) (Hanabi_Env.py:451-500) as two launches: one thread per table
 * applies actions[n] (device int32: move uid, or -1 to sit the move out) and deals (at most players * hand_size cards)
 * until a player is to move, writing rewards [n] float32 (score differential), status [n] uint8, scores [n] int32 and
 * flags; then one workgroup per table encodes the rows of the player now to move (zero rows for idle and refused
 * tables).  UNLIKE the host call, which validates all moves first and applies none if one is illegal, an illegal or
 * out-of-range uid -- or a table that was never reset -- leaves THAT table untouched and reports status 255 in its
 * flags / status while the other tables advance: the caller reads the flags back and raises. */
int mappo_hanabi_step(void* state, const int32_t* actions, float* rewards, uint8_t* status, int32_t* scores, float* obs,
                      float* share_obs, float* available, int32_t* to_move, int32_t* flags, int64_t n_tables,
                      int share_mode, int32_t colors, int32_t ranks, int32_t players, int32_t hand_size,
                      int32_t max_information_tokens, int32_t max_life_tokens, int32_t observation_type,
                      int32_t random_start_player, mappo_stream_t stream);

/* hanabi_batch_encode alone: the rows of every started table with active[n] != 0 (device uint8; NULL: all), zero rows
 * for the others (canonical_encoders.cc, sections as listed above).  One launch. */
int mappo_hanabi_encode(const void* state, const uint8_t* active, float* obs, float* share_obs, float* available,
                        int32_t* to_move, int64_t n_tables, int share_mode, int32_t colors, int32_t ranks,
                        int32_t players, int32_t hand_size, int32_t max_information_tokens, int32_t max_life_tokens,
                        int32_t observation_type, int32_t random_start_player, mappo_stream_t stream);

/* draws[n] int32 (device): 32-bit words each table's generator has produced since mappo_hanabi_seed (tests, tools). */
int mappo_hanabi_draws(const void* state, int32_t* draws, int64_t n_tables, mappo_stream_t stream);

/* ------------------------------------------------- K17: the turn bookkeeping of a Hanabi move, from the flags words ----
 * What HanabiRunner.collect does around the env step of one player's move (reference
 * onpolicy/runner/shared/hanabi_runner_forward.py:138-220: the masked numpy assignments on the arrays shaped like a buffer
 * row, the choose / reset_choose decisions, the score list, true_total_num_steps) as two launches that read "who moves"
 * and "which games ended" off device memory -- bit 8 and the status byte of K16's flags words -- so that a move needs no
 * device -> host copy.  All operands of one move travel in one descriptor:
 *   turn tensors, contiguous [n_tables, players, W] float32 (W = obs_w / share_w / avail_w for the three row fields, 1 for
 *     the others): obs, share_obs, available_actions, values, actions, action_log_probs, rewards,
 *     rewards_since_last_action, masks, active_masks;
 *   current rows [n_tables, W]: use_obs, use_share_obs (may alias use_obs), use_available_actions;
 *   the policy's outputs [n_tables]: value, action (int64), logp;   the env's: flags (int32, K16), rewards_env;
 *   the route's state [n_tables]: can_move (int32), reset_choose (uint8), env_actions (int32), and the per-table
 *     accumulators moves (int64), games, score_sum (int32), refused (uint8) -- summed on the host, so nothing is atomic
 *     and nothing depends on order.
 * The six row arrays must be 16-byte aligned, moves and action 8-byte, everything else 4-byte (uint8 arrays: any).
 *
 * mappo_hanabi_turn_begin(agent), per table n with m = can_move[n] != 0:
 *   env_actions[n] = m ? (int32) action[n] : -1;  if m: rows [n, agent] of obs / share_obs / available_actions = the
 *   current rows of n, values[n, agent] = value[n], actions[n, agent] = (float) action[n],
 *   action_log_probs[n, agent] = logp[n].  A table that sits out has nothing else written.
 * mappo_hanabi_turn_end(agent), per table n with status = flags[n] & 0xff, m as turn_begin read it, in this order:
 *   if m:            rewards[n, agent] = rsla[n, agent]; rsla[n, agent] = 0; rsla[n, a] += rewards_env[n] for every a;
 *                    moves[n] += 1                                   (rsla = rewards_since_last_action)
 *   if status == 0:  masks[n, agent] = active_masks[n, agent] = 1
 *   if status == 1:  reset_choose[n] = 1; games[n] += 1; score_sum[n] += flags[n] >> 16; row n of use_available_actions
 *                    = 0; masks[n, :] = 0; active_masks[n, agent] = 1; for every a > agent: active_masks[n, a] = 0,
 *                    rewards[n, a] = rsla[n, a], rsla[n, a] = 0, values[n, a] = 0, rows [n, a] of obs and share_obs = 0
 *   if status == 255: refused[n] = 1 (sticky)
 *   can_move[n] = status == 1 ? 0 : (flags[n] >> 8) & 1
 * One wave per table, at most MAPPO_TURN_MAX_BLOCKS workgroups of four waves striding over the tables; rows are moved
 * 16 bytes per lane wherever source and destination share their offset from a 16-byte boundary (else 4-byte loads,
 * 16-byte stores).  MAPPO_E_NULL (a pointer the call reads or writes; the other call's may be NULL), MAPPO_E_SHAPE (n_tables <= 0, players outside [1, 5], agent outside
 * [0, players), a width <= 0) and MAPPO_E_ALIGN are returned before anything is enqueued. */
#define MAPPO_TURN_MAX_BLOCKS 2048
#define MAPPO_TURN_MAX_PLAYERS 5
typedef struct mappo_hanabi_turn {
    float* obs;
    float* share_obs;
    float* available_actions;
    float* values;
    float* actions;
    float* action_log_probs;
    float* rewards;
    float* rewards_since_last_action;
    float* masks;
    float* active_masks;
    float* use_obs;
    float* use_share_obs;
    float* use_available_actions;
    const float* value;
    const int64_t* action;
    const float* logp;
    const int32_t* flags;
    const float* rewards_env;
    int32_t* can_move;
    uint8_t* reset_choose;
    int32_t* env_actions;
    int64_t* moves;
    int32_t* games;
    int32_t* score_sum;
    uint8_t* refused;
    int64_t n_tables;
    int32_t players;
    int32_t obs_w;
    int32_t share_w;
    int32_t avail_w;
} mappo_hanabi_turn_t;
int mappo_hanabi_turn_begin(const mappo_hanabi_turn_t* args, int agent, mappo_stream_t stream);
int mappo_hanabi_turn_end(const mappo_hanabi_turn_t* args, int agent, mappo_stream_t stream);

/* K17 for a recurrent policy: the same two launches, which also keep the two RNN state tensors of the turn (what
 * HanabiRunner.collect does with turn_rnn_states / turn_rnn_states_critic around the env step, same reference lines).  The
 * descriptor is K17's, field for field, followed by
 *   rnn_states, rnn_states_critic, contiguous [n_tables, players, rnn_w] float32 (rnn_w = recurrent_N * hidden_size): the
 *     actor's and the critic's state per (table, player);
 *   rnn_new, rnn_new_critic [n_tables, rnn_w]: the policy's new states on ALL rows.
 * These four must be 16-byte aligned; a slot row sits at (n * players + agent) * rnn_w floats, rnn_w need not be a multiple
 * of four.  K17's requirements hold for the other operands.
 *
 * mappo_hanabi_turn_begin_rnn(agent), per table n with m = can_move[n] != 0: everything mappo_hanabi_turn_begin does, then
 *   if m: rnn_states[n, agent, :] = rnn_new[n, :]; rnn_states_critic[n, agent, :] = rnn_new_critic[n, :].
 *   A table that sits out keeps both states: what the policy computed for it is discarded.
 * mappo_hanabi_turn_end_rnn(agent), per table n: everything mappo_hanabi_turn_end does, in its order, then
 *   if status == 1:  rnn_states[n, a, :] = rnn_states_critic[n, a, :] = 0 for EVERY player a (not only a > agent).
 * One launch each, K17's kernels instantiated on this descriptor.  MAPPO_E_NULL (a pointer the call reads or writes: all
 * four state pointers in _begin_rnn; in _end_rnn the two state tensors -- rnn_new / rnn_new_critic may be NULL there),
 * MAPPO_E_SHAPE (K17's cases; rnn_w <= 0 or rnn_w > INT32_MAX / 5) and MAPPO_E_ALIGN (K17's cases; one of the four state
 * arrays not 16-byte aligned) are returned before anything is enqueued. */
typedef struct mappo_hanabi_turn_rnn {
    float* obs;
    float* share_obs;
    float* available_actions;
    float* values;
    float* actions;
    float* action_log_probs;
    float* rewards;
    float* rewards_since_last_action;
    float* masks;
    float* active_masks;
    float* use_obs;
    float* use_share_obs;
    float* use_available_actions;
    const float* value;
    const int64_t* action;
    const float* logp;
    const int32_t* flags;
    const float* rewards_env;
    int32_t* can_move;
    uint8_t* reset_choose;
    int32_t* env_actions;
    int64_t* moves;
    int32_t* games;
    int32_t* score_sum;
    uint8_t* refused;
    float* rnn_states;
    float* rnn_states_critic;
    const float* rnn_new;
    const float* rnn_new_critic;
    int64_t n_tables;
    int32_t players;
    int32_t obs_w;
    int32_t share_w;
    int32_t avail_w;
    int32_t rnn_w;
} mappo_hanabi_turn_rnn_t;
int mappo_hanabi_turn_begin_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream);
int mappo_hanabi_turn_end_rnn(const mappo_hanabi_turn_rnn_t* args, int agent, mappo_stream_t stream);

/* ------------------------------------------------- K18: the bookkeeping of a Hanabi EVALUATION move, from the flags words ----
 * What HanabiRunner.eval does around the env step of one player's move (reference
 * onpolicy/runner/shared/hanabi_runner_forward.py:229 onwards: the choose mask, the -1 actions of the tables that sit out,
 * eval_rnn_states[choose, agent_id] = ..., eval_available_actions[eval_dones == True] = 0, the eval_scores list) as two
 * launches in K17's shape that read "who moves" and "which games ended" off device memory, so that an evaluation move needs
 * no device -> host copy.  Evaluation bookkeeping is not training bookkeeping: no buffer slots, rewards or masks; per-table
 * final scores; RNN state carried per (table, player) through a whole game; finished tables are never restarted.
 *   current rows [n_tables, avail_w] float32: use_available_actions;
 *   rnn_states [n_tables, players, rnn_w] float32 (rnn_w = recurrent_N * hidden), rnn_new [n_tables, rnn_w]: the policy's new
 *     states on all rows -- BOTH NULL for a feed-forward policy (rnn_w is ignored then);
 *   the policy's action [n_tables] int64; the env's flags [n_tables] int32 (K16);
 *   the route's state [n_tables]: can_move, env_actions (int32), and the per-table counters moves (int64), games, scores
 *     (int32), refused (uint8).
 * use_available_actions, rnn_states and rnn_new must be 16-byte aligned, moves and action 8-byte, the others 4-byte.
 *
 * mappo_hanabi_eval_begin(agent), per table n with m = can_move[n] != 0:
 *   env_actions[n] = m ? (int32) action[n] : -1;  if m and the RNN pointers are set: rnn_states[n, agent, :] = rnn_new[n, :].
 *   A table that sits out keeps its state: what the policy computed for it is discarded.
 * mappo_hanabi_eval_end(agent), per table n with f = flags[n], status = f & 0xff, m as eval_begin read it:
 *   if m:                 moves[n] += 1
 *   if m and status == 1: scores[n] = f >> 16; games[n] += 1; row n of use_available_actions = 0
 *   if status == 255:     refused[n] = 1 (sticky)
 *   can_move[n] = (m && status == 0) ? (f >> 8) & 1 : 0
 * A finished table is counted once and never moves again (K16 reports it as status 2 with zero rows from then on).
 * MAPPO_E_NULL (a pointer the call reads or writes; the other call's may be NULL; one RNN pointer without the other),
 * MAPPO_E_SHAPE (n_tables <= 0, players outside [1, 5], agent outside [0, players), avail_w <= 0, rnn_w <= 0 with the RNN
 * pointers set) and MAPPO_E_ALIGN are returned before anything is enqueued. */
typedef struct mappo_hanabi_eval {
    float* use_available_actions;
    float* rnn_states;
    const float* rnn_new;
    const int64_t* action;
    const int32_t* flags;
    int32_t* can_move;
    int32_t* env_actions;
    int64_t* moves;
    int32_t* games;
    int32_t* scores;
    uint8_t* refused;
    int64_t n_tables;
    int32_t players;
    int32_t avail_w;
    int32_t rnn_w;
} mappo_hanabi_eval_t;
int mappo_hanabi_eval_begin(const mappo_hanabi_eval_t* args, int agent, mappo_stream_t stream);
int mappo_hanabi_eval_end(const mappo_hanabi_eval_t* args, int agent, mappo_stream_t stream);

/* --------------------------------------------------------------------- misc ---- */
int         mappo_abi_version(void);
const char* mappo_build_info(void);        /* "gfx950 ..." static string */
const char* mappo_error_string(int code);  /* static string for a return code */

#ifdef __cplusplus
}
#endif
#endif /* MAPPO_HIP_H */

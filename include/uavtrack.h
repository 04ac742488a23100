/*
 * uavtrack.h -- C ABI of libuavtrack.so, the MI355X (gfx950) batched
 * multi-UAV target-tracking environment.
 *
 * The reference (tjuDavidWang/MARL-UAVs-Targets-Tracking) has no FFI: its hot
 * path is the duck-typed Python class `Environment` (src/environment.py:12).
 * Each entry point below names the reference interface it replaces; the Python
 * binding a maintainer adds on the reference side is in INTEGRATION.md and is
 * what marl-uavs-targets-tracking_amd/uavtrack/_lib.py implements (ctypes).
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on failure; the message is
 *    in uavtrack_last_error() (thread-local).  No exceptions cross the ABI.
 *  - all array arguments are DEVICE pointers (HIP), caller-owned, contiguous,
 *    fp32 / int32 / uint8 as declared.  The library keeps no reference to them
 *    after the stream work it enqueued has run.
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream).
 *    The stepping and reset calls are asynchronous on that stream and never
 *    synchronise the host or allocate: they can be captured into a HIP graph.
 *    (MAAC-R scratch is sized for cfg.horizon steps when the weights are set;
 *    only a longer call grows it -- a synchronisation -- and under capture
 *    that call is refused instead.)  The calls that DO synchronise say so:
 *    the weight uploads, the info / accounting queries, uavtrack_step_host.
 *  - a handle is owned by one host thread at a time (like the reference's
 *    single-threaded Environment); one handle per GPU, one process per GPU.
 *  - batch layout is struct-of-arrays: UAV arrays are [n_envs][n_uav], target
 *    arrays [n_envs][m_targets], row-major, environment-major.
 *  - there is no CPU fallback: on a machine without a gfx950 device
 *    uavtrack_create fails.
 */
#ifndef UAVTRACK_H
#define UAVTRACK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UAVTRACK_ABI_VERSION 1
#define UAVTRACK_OBS_DIM 12      /* environment.py:28  state_dim = (4+1) + 4 + (2+1) */
#define UAVTRACK_MAX_CLIMB 8

/* Which cooperative reward runs in Environment.calculate_rewards
 * (environment.py:222-226 -> uav.py:312-322). */
enum uavtrack_reward_mode {
    UAVTRACK_REWARD_RAW  = 0,   /* MAAC:   cooperative == 0, reward = raw      (uav.py:270,300) */
    UAVTRACK_REWARD_MEAN = 1,   /* MAAC-G: pmi is None, neighbour mean         (uav.py:293-310) */
    UAVTRACK_REWARD_PMI  = 2    /* MAAC-R: PMI-softmax weighted neighbours     (uav.py:262-291) */
};

/* Everything Environment.__init__ (environment.py:13-43), Environment.reset
 * (environment.py:87-107) and the per-step `config` dict reads
 * (environment.py:207-224) -- captured once, as a POD. */
typedef struct uavtrack_config {
    uint32_t struct_size;       /* = sizeof(uavtrack_config), ABI check */
    int32_t  n_envs;            /* B: independent Environment instances on this GPU */
    int32_t  n_uav;             /* environment.n_uav      (environment.py:32) */
    int32_t  m_targets;         /* environment.m_targets  (environment.py:33) */
    int32_t  dim;               /* 2 (reference) or 3 (our own spec) */
    int32_t  na;                /* environment.na, turn-rate actions (uav.py:73-81) */
    int32_t  nc;                /* climb-angle actions, 1 in 2-D; action = a_turn + na * a_climb */
    int32_t  norm_n_uav;        /* config['environment']['n_uav'] of the clip   (environment.py:210) */
    int32_t  norm_m_targets;    /* config['environment']['m_targets'] of the clip (environment.py:208) */
    int32_t  reward_mode;       /* enum uavtrack_reward_mode */
    int32_t  horizon;           /* done[b] = step_count[b] >= horizon (train.py:160 num_steps); 0 = never */
    int32_t  device_id;         /* HIP device ordinal */
    int64_t  env_offset;        /* global id of env 0 of this shard (keys the reset RNG; multi-GPU) */
    double   x_max, y_max, z_max;
    double   dt;                /* uav.dt */
    double   u_v_max;           /* uav.v_max */
    double   u_h_max;           /* radians: pi / yaml uav.h_max (environment.py:100) */
    double   u_g_max;           /* radians: max climb angle (3-D only) */
    double   dc, dp;            /* uav.dc, uav.dp */
    double   t_v_max;           /* target.v_max */
    double   alpha, beta, gamma;/* uav.alpha/beta/gamma (environment.py:219-220) */
    double   cooperative;       /* config['cooperative'] (environment.py:224) */
} uavtrack_config;

typedef struct uavtrack_env uavtrack_env;   /* opaque handle */

/* ABI version of the loaded library. */
int uavtrack_version(void);

/* Message of the last failure on this thread ("" if none). */
const char *uavtrack_last_error(void);

/* Replaces Environment.__init__ (environment.py:13-43).  Allocates the
 * internal SoA state on cfg->device_id.  Fails if no gfx950 device. */
int uavtrack_create(const uavtrack_config *cfg, uavtrack_env **out);

/* Frees the handle and its device state. */
int uavtrack_destroy(uavtrack_env *env);

/* Replaces Environment.reset (environment.py:87-107): UAV i (1-based) at
 * x = i*x_max/(n_uav+1), y = y_max/2 [, z = z_max/2], heading ~ U(-pi,pi),
 * previous action ~ U{0..na*nc-1}; targets uniform in the box, heading
 * ~ U(-pi,pi).  The reference draws from Python's MT19937; here the stream is
 * Philox4x32-10 keyed by (seed, env_offset + b, episode, agent), so a shard
 * reproduces the same envs as the unsharded batch.  step_count <- 0.
 * obs (nullable) [B][N][12] receives get_states() of the fresh state:
 * [-1]*9 + [x/dc, y/dc, a/Na] (uav.py:174,186). */
int uavtrack_reset(uavtrack_env *env, uint64_t seed, uint32_t episode,
                   float *obs, void *stream);

/* State injection / extraction (no reference equivalent: the reference pokes
 * uav.x / target.x attributes directly; used for parity tests and as the env
 * checkpoint).  uz/tz are ignored (may be NULL) when dim == 2.  step_count
 * (nullable) is int32[B]. */
int uavtrack_set_state(uavtrack_env *env,
                       const float *ux, const float *uy, const float *uz, const float *uh,
                       const int32_t *ua,
                       const float *tx, const float *ty, const float *tz, const float *th,
                       const int32_t *step_count, void *stream);
int uavtrack_get_state(uavtrack_env *env,
                       float *ux, float *uy, float *uz, float *uh, int32_t *ua,
                       float *tx, float *ty, float *tz, float *th,
                       int32_t *step_count, void *stream);

/* The rest of the checkpoint: episode [B] int32 (device pointer) = the number of each environment's last reset
 * (uavtrack_reset's `episode` argument, advanced by every automatic reset).  It keys the Philox counter of the next
 * automatic reset (uavtrack_step_many_autoreset), so a handle restored with uavtrack_set_state + uavtrack_set_episodes
 * resets into the same states as the run the checkpoint was taken from.  (A separate pair of entry points: the
 * signatures of uavtrack_set_state / uavtrack_get_state stay as they are.) */
int uavtrack_set_episodes(uavtrack_env *env, const int32_t *episode, void *stream);
int uavtrack_get_episodes(uavtrack_env *env, int32_t *episode, void *stream);

/* Replaces the `pmi` argument of Environment.step (environment.py:120;
 * PMINetwork.inference PMINet.py:64-72, eval mode).  `folded` is a HOST
 * pointer to the BatchNorm-folded fp32 blob, layout (H = hidden):
 *   Wc[5][H] bc[H]  Wo[4][H] bo[H]  Wb[3][H] bb[H]  W1[3H][H] b1[H]  w2[H] b2[1]
 * (input-major so consecutive lanes read consecutive outputs).  n_floats must
 * equal 12H + 3H + 3H*H + H + H + 1.  folded == NULL disables PMI. */
int uavtrack_set_pmi_weights(uavtrack_env *env, const float *folded, size_t n_floats,
                             int32_t hidden, void *stream);

/* Which arithmetic scores the neighbour pairs (the 3H x H layer of PMINet.py:59, 98 % of the network's work).  All
 * three evaluate PMINetwork.forward at fp32 accuracy (tested against an fp64 forward); they differ in speed and range:
 *   F16X3   three f16 MFMAs per fp32 product on block-scaled operand planes -- the default for hidden 64 / 96 / 128 when
 *           the weights and the activation bounds fit f16's range; it watches its inputs, and a chunk in which an operand
 *           could saturate is scored again by BF16X6 (stream-ordered, counted in uavtrack_pmi_info);
 *   BF16X6  six bf16 MFMAs per fp32 product: fp32's exponent range -- networks the range guard turns away;
 *   FP32    fp32-input MFMA: every width up to 256 (the only kernel for 32 and for widths past 128). */
enum uavtrack_pmi_scheme {
    UAVTRACK_PMI_AUTO   = 0,    /* the fastest one the weights allow (the default) */
    UAVTRACK_PMI_F16X3  = 1,
    UAVTRACK_PMI_BF16X6 = 2,
    UAVTRACK_PMI_FP32   = 3
};

/* Pins the scorer (A/B measurements, parity tests of every dispatchable kernel).  Fails when the loaded weights
 * cannot run on that scheme (width, or f16 range); uavtrack_set_pmi_weights fails likewise while a scheme is pinned. */
int uavtrack_set_pmi_scheme(uavtrack_env *env, int32_t scheme);

/* out[0] = the scheme the next MAAC-R step / uavtrack_pmi_inference will launch (enum uavtrack_pmi_scheme, never AUTO;
 * 0 without weights), out[1] = the hidden width after padding to a multiple of 32, out[2] = 1 if the weights passed the
 * host-side f16 range guard, out[3] = chunks the wide-range kernel has re-scored since the handle was created because an
 * operand left f16's range at run time.  Synchronises `stream`. */
int uavtrack_pmi_info(uavtrack_env *env, int64_t out[4], void *stream);

/* The 26 fp32 tensors of a PMINetwork (PMINet.py:20-62) as DEVICE pointers in torch layouts: the four Linear +
 * BatchNorm1d blocks in the order fc_comm / bn_comm (in = 5), fc_obs / bn_obs (4), fc_boundary_state /
 * bn_boundary_state (3), fc1 / bn1 (3 hidden) -- weight [hidden][in], bias, BatchNorm weight, bias, running_mean,
 * running_var [hidden] each -- then fc2.weight [1][hidden] and fc2.bias [1]. */
typedef struct uavtrack_pmi_tensors {
    struct {
        const float *weight, *bias, *bn_weight, *bn_bias, *running_mean, *running_var;
    } block[4];
    const float *fc2_weight, *fc2_bias;
} uavtrack_pmi_tensors;

/* uavtrack_set_pmi_weights without the host: BatchNorm fold (fp64, each result rounded once to fp32, as
 * uavtrack/pmi.py folds), padding, bounds, block scales, range-watch limits, the f16 verdict and all packed layouts
 * are computed on the device from the tensors of `t`, bitwise identical to what the host path writes from the same
 * numbers (csrc/pmi_pack.h states every rounding once, for both).  Stream-ordered: no synchronisation, no allocation,
 * capturable into a graph; the tensors are read when the launches execute on `stream`, not when this is called.  The
 * handle must already hold weights of the same `hidden` (uavtrack_set_pmi_weights sizes the allocation and the
 * scratch).  Returns an error, enqueuing nothing and leaving the installed weights in place, for a null pointer, no
 * weights installed, or `hidden` other than the installed width.
 * At widths 64 / 96 / 128 the verdict "fits f16's range" is then known to the device only: from this call until the
 * next uavtrack_set_pmi_weights the handle launches F16X3 with its gated BF16X6 stand-by under AUTO and F16X3 alike;
 * weights that do not fit are scored by the stand-by -- the BF16X6 scores of the host path, bit for bit -- and such
 * chunks are counted in uavtrack_pmi_publish_info, not in uavtrack_pmi_info's out[3].  A scheme pinned to F16X3 can
 * therefore not be refused by a device publish; uavtrack_pmi_info reports BF16X6 while the verdict is "unfit". */
int uavtrack_publish_pmi_weights(uavtrack_env *env, const uavtrack_pmi_tensors *t, int32_t hidden, void *stream);

/* out[0] = 1 if the installed weights come from a device publish (0 after uavtrack_set_pmi_weights), out[1] = chunks
 * the wide-range kernel has scored since the handle was created because device-published weights did not fit f16's
 * range (the run-time range watch keeps its own count, uavtrack_pmi_info out[3]).  Synchronises `stream`. */
int uavtrack_pmi_publish_info(uavtrack_env *env, int64_t out[2], void *stream);

/* Inspection aid: the size in floats of the installed weights allocation (0 without weights), and a copy of all of it
 * -- the fp32 blob in scorer order, the bf16 / f16 planes of widths 64 / 96 / 128, the 8-word scalar block
 * (csrc/pmi_pack.h) -- to a HOST buffer of exactly that many floats.  The copy synchronises `stream`. */
int uavtrack_pmi_blob_floats(uavtrack_env *env, int64_t *out);
int uavtrack_get_pmi_blob(uavtrack_env *env, float *host, int64_t n_floats, void *stream);

/* Replaces PMINetwork.inference (PMINet.py:64-72: eval mode, no grad) on a batch: x [n][12] (device; row k is what
 * uav.py:281 builds, la_i * la_j) -> scores [n] (device), with the weights of uavtrack_set_pmi_weights and on the very
 * kernels that score the neighbour pairs of a MAAC-R step (f16 x 3 on block-scaled planes, bf16 x 6 or fp32 MFMA by width and weight range) -- the network alone, for
 * callers that hold pair inputs of their own and for accuracy tests of the scorer.  Stream-ordered; must not run
 * concurrently with a MAAC-R step of the same handle.  (Not counted by uavtrack_pmi_pairs_scored.) */
int uavtrack_pmi_inference(uavtrack_env *env, const float *x, int64_t n, float *scores, void *stream);

/* Replaces Environment.step (environment.py:120-164) for the whole batch.
 *   actions [B][N] int32 in [0, na*nc)      (train.py:173-176 action_list)
 *   obs     [B][N][12]  next_states          (environment.py:144)
 *   reward  [B][N]      reward['rewards']    (environment.py:158)
 *   terms   [3][B][N]   target_tracking_reward, boundary_punishment,
 *                       duplicate_tracking_punishment (environment.py:159-161); nullable
 *   covered [B] int32   covered_targets      (environment.py:146); nullable
 *   done    [B] uint8   step_count >= horizon; nullable */
int uavtrack_step(uavtrack_env *env, const int32_t *actions,
                  float *obs, float *reward, float *terms,
                  int32_t *covered, uint8_t *done, void *stream);

/* T consecutive steps in ONE launch with the state resident on chip
 * (replaces the `for i in range(num_steps)` loop of train.py:160-185 for
 * open-loop / pre-sampled actions).  Bitwise identical to T uavtrack_step
 * calls.  Outputs gain a leading [T] axis: actions [T][B][N], obs
 * [T][B][N][12], reward [T][B][N], terms [T][3][B][N], covered [T][B],
 * done [T][B].  ep_sums (nullable) [B][5] receives the episode accumulators of
 * train.py:181-192 over the T steps: sum_t mean_i reward, sum_t mean_i of the
 * three terms, sum_t covered. obs/terms/covered/done/ep_sums are nullable. */
int uavtrack_step_many(uavtrack_env *env, int32_t T, const int32_t *actions,
                       float *obs, float *reward, float *terms,
                       int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* uavtrack_step_many with automatic episode turnover (rollouts of T steps "with auto-reset at done"): an
 * environment whose done flag fires at step t (step_count reached cfg.horizon) is reset right behind that step, inside
 * the launch -- exactly uavtrack_reset(reset_seed, e + 1) for that environment, e being the episode number of its
 * previous reset (uavtrack_reset stores its `episode` argument per environment) -- so one launch may span episodes
 * and the driver's per-episode reset launch disappears.  Row t of the outputs is the terminal step, as without the
 * reset; row t + 1 is the first step of the new episode (the reset state's own observation, [-1]*9 + [x/dc, y/dc, a/Na],
 * is not emitted; an in-kernel policy sees it).  Bitwise identical to: uavtrack_step_many up to each done step,
 * uavtrack_reset, continue.  ep_sums runs over the whole call.  Needs cfg.horizon >= 1. */
int uavtrack_step_many_autoreset(uavtrack_env *env, int32_t T, uint64_t reset_seed, const int32_t *actions,
                                 float *obs, float *reward, float *terms,
                                 int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* uavtrack_step that also ADDS this step's contribution to the caller's running episode
 * accumulators ep_sums [B][5] (same five sums as uavtrack_step_many, train.py:181-192), so a
 * closed-loop driver needs no reduction kernels of its own.  ep_sums must not be NULL. */
int uavtrack_step_accumulate(uavtrack_env *env, const int32_t *actions,
                             float *obs, float *reward, float *terms,
                             int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* Replaces UAV.get_action_by_direction (uav.py:324-369), the C-METHOD greedy baseline policy, for
 * every UAV on the current state: actions [B][N] int32 out.  score_t = 1/d(u,t) - 0.8 * #{other UAVs
 * within dc of t}, first best target, angle = atan2 - heading, epsilon 0.25 random action, 0.3
 * keep-straight.  The reference calls an undefined find_closest_a_idx (uav.py:368); here it is the
 * turn rate of uav.py:73-81 nearest to the wrapped angle (lowest index on ties).  Draws are Philox
 * keyed by (seed, env_offset + b, step_count[b], uav).  2-D only. */
int uavtrack_greedy_actions(uavtrack_env *env, uint64_t seed, int32_t *actions, void *stream);

/* The whole C-METHOD evaluation loop of train.run_epoch (train.py:326-370) in ONE launch: per step the
 * baseline policy above picks the actions from the current state, then Environment.step runs -- T
 * closed-loop steps with the state on chip.  Bitwise identical to T x (uavtrack_greedy_actions,
 * uavtrack_step).  actions_out (nullable) [T][B][N] receives the chosen actions; the other outputs are
 * those of uavtrack_step_many.  Reward modes RAW / MEAN, 2-D only. */
int uavtrack_run_greedy(uavtrack_env *env, int32_t T, uint64_t seed, int32_t *actions_out,
                        float *obs, float *reward, float *terms,
                        int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* ---- the learner's shared actor, run on the device next to the environment ----
 * The reference's train.operate_epoch calls ActorCritic.take_action once per UAV per step
 * (train.py:165-172 -> actor_critic.py:138-148): a batch-1 forward of FnnPolicyNet
 * (actor_critic.py:85-98: Linear(12,H) - ReLU - Linear(H,na) - softmax) and Categorical(probs).sample(),
 * with a host round trip each.  These three entry points keep that loop on the GPU. */
enum { UAVTRACK_ACTOR_SAMPLE = 0,   /* Categorical(probs).sample(): inverse CDF at a Philox uniform */
       UAVTRACK_ACTOR_ARGMAX = 1 }; /* deterministic evaluation: most probable action, lowest index on ties */

/* Uploads FnnPolicyNet's parameters (HOST pointers, fp32, torch layouts): w1 [hidden][12] = fc1.weight,
 * b1 [hidden] = fc1.bias, w2 [na*nc][hidden] = fc2.weight, b2 [na*nc] = fc2.bias.  na <= 12 in 2-D (the
 * reference's action space, configs: na = 12), na*nc <= 48 in 3-D.  w1 = NULL removes the actor.
 * Synchronises `stream`. */
int uavtrack_set_actor_weights(uavtrack_env *env, const float *w1, const float *b1,
                               const float *w2, const float *b2, int32_t hidden, void *stream);

/* The same upload from DEVICE pointers (fp32, the torch layouts above), without the host: the blob is packed on the
 * device, bitwise identical to what uavtrack_set_actor_weights packs from the same weights (up to the one case named
 * in csrc/actor_pack_kernel.hip: a scale ratio within an ulp or two of a power of two, where the host's and the
 * device's log2 may floor apart).  Stream-ordered: no synchronisation, no allocation, capturable into a graph; the
 * weights are read when the launches execute on `stream`, not when this is called.  The handle must already hold an
 * actor of the same `hidden` (uavtrack_set_actor_weights sizes the blob).  Returns an error, enqueuing nothing and
 * leaving the installed weights in place, for a null pointer, no actor installed, `hidden` other than the installed
 * width, or na*nc beyond what the device actor holds. */
int uavtrack_publish_actor_weights(uavtrack_env *env, const float *w1, const float *b1,
                                   const float *w2, const float *b2, int32_t hidden, void *stream);

/* Inspection aid: copies the installed actor blob (csrc/actor.h layout) to a HOST buffer of n_floats floats, which
 * must equal the blob's size (128 + ceil(hidden / 32) * (2 + 4 AT) * 256, AT = 1 in 2-D, 2 in 3-D).  Synchronises
 * `stream`.  Fails if no actor is installed. */
int uavtrack_get_actor_blob(uavtrack_env *env, float *host, int64_t n_floats, void *stream);

/* take_action for every UAV: obs [B][N][12] (what get_local_state returned, i.e. the obs output of the
 * previous step / reset) -> actions [B][N] int32, and, if probs != NULL, the policy's probabilities
 * probs [B][N][na*nc].  Draws: Philox4x32-10 keyed by seed, counter (env_offset + b, step_count[b] >> 2,
 * uav); the uniform of step s is word s & 3 of that block (24 bits), the action the first index whose
 * cumulative probability exceeds it. */
int uavtrack_actor_actions(uavtrack_env *env, const float *obs, uint64_t seed, int32_t mode,
                           int32_t *actions, float *probs, void *stream);

/* The rollout half of train.operate_epoch (train.py:160-192) in ONE launch: per step every UAV's action
 * comes from the actor applied to its own previous observation (held in registers), then
 * Environment.step runs -- T closed-loop steps with the state on chip.  obs_in [B][N][12] is the
 * observation the policy sees at the first step.  Bitwise identical to T x (uavtrack_actor_actions,
 * uavtrack_step).  actions_out (nullable) [T][B][N]; the other outputs are those of uavtrack_step_many,
 * i.e. the (state, action, reward, next_state) transitions of train.py:176-180 land in
 * obs[t-1] / actions_out[t] / reward[t] / obs[t].  With reward_mode PMI the launch is chunked like
 * uavtrack_step_many (rollout, pair scorer, softmax mix per chunk); the policy never reads rewards. */
int uavtrack_run_actor(uavtrack_env *env, int32_t T, uint64_t seed, int32_t mode, const float *obs_in,
                       int32_t *actions_out, float *obs, float *reward, float *terms,
                       int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* uavtrack_run_actor with the automatic episode turnover of uavtrack_step_many_autoreset: one launch of the fused
 * policy rollout may span any number of episodes.  An environment whose done flag fires at step t is reset right behind
 * that step -- exactly uavtrack_reset(reset_seed, e + 1), e the episode number of its previous reset -- and the actor's
 * input at step t + 1 is the fresh state's observation ([-1]*9 + [x/dc, y/dc, a/Na], uavtrack_reset's obs output).
 * The draw stream: while an environment is in episode e (what uavtrack_reset stored, plus the resets of this launch so
 * far), its draws use the Philox key of seed + e (mod 2^64); a cached Philox block never crosses a reset.
 * The equivalence the tests hold the call to -- bitwise, per environment: uavtrack_run_actor with seed + e up to each
 * done step, then uavtrack_reset(reset_seed, e + 1), then uavtrack_run_actor with seed + e + 1 from the reset's
 * observation, and so on; ep_sums runs over the whole call.  Everything else is uavtrack_run_actor's contract plus
 * uavtrack_step_many_autoreset's: needs cfg.horizon >= 1; stream-ordered, no allocation, no synchronisation, capturable;
 * with reward_mode PMI the launch is chunked as uavtrack_run_actor is.  Every reward mode, 2-D and 3-D.  Returns an
 * error, enqueuing nothing, for what uavtrack_run_actor refuses, for cfg.horizon < 1, and for a start-observation buffer
 * (below) that holds fewer than T steps. */
int uavtrack_run_actor_autoreset(uavtrack_env *env, int32_t T, uint64_t seed, uint64_t reset_seed, int32_t mode,
                                 const float *obs_in, int32_t *actions_out, float *obs, float *reward, float *terms,
                                 int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* uavtrack_run_greedy with the same turnover and the same draw-stream rule (key of seed + e in episode e).  Bitwise
 * identical, per environment, to: uavtrack_run_greedy with seed + e up to each done step, uavtrack_reset(reset_seed,
 * e + 1), continue.  uavtrack_run_greedy's own limits stay: a 3-D configuration or reward_mode PMI is refused with an
 * error that names the combination (there is no rollout kernel for it). */
int uavtrack_run_greedy_autoreset(uavtrack_env *env, int32_t T, uint64_t seed, uint64_t reset_seed, int32_t *actions_out,
                                  float *obs, float *reward, float *terms,
                                  int32_t *covered, uint8_t *done, float *ep_sums, void *stream);

/* Optional extra output of the automatic-reset entry points (uavtrack_step_many_autoreset, _run_actor_autoreset,
 * _run_greedy_autoreset), installed like the raw rewards below: start_obs [T][B][N][12].  Row (t, b) is written only
 * where done[t][b] fired, and holds the observation of the fresh state the environment was reset to -- the policy's
 * input at step t + 1, the `state` of the transition at t + 1 (uavtrack_replay_add_rollout_episodes); every other row
 * is left untouched.  Launches without the automatic reset never see the buffer.  A device pointer, 16-byte aligned;
 * capacity_steps >= the largest T passed to an automatic-reset call while the buffer is set (checked);
 * start_obs = NULL switches the output off (the default). */
int uavtrack_set_start_obs_output(uavtrack_env *env, float *start_obs, int32_t capacity_steps);

/* Optional extra output of every stepping entry point (uavtrack_step, _step_accumulate, _step_many, _run_greedy,
 * _run_actor): the target positions after each step, tpos [T][B][M][2] = (x, y) -- what Environment.step appends to
 * position['all_target_xs'/'all_target_ys'] (environment.py:150-153) and Environment.save_position writes to
 * t_xy<ep>.csv (environment.py:232-238).  (UAV positions are already in the observations: obs[..., 9:11] * dc,
 * uav.py:154.)  The buffer, a device pointer like the others, is written by every later stepping call -- row t of the
 * call's T steps at tpos[t] -- until it is replaced; it must hold capacity_steps >= the largest T passed while it
 * is set (checked).  tpos = NULL switches the output off (the default). */
int uavtrack_set_target_trace(uavtrack_env *env, float *tpos, int32_t capacity_steps);

/* Optional extra output of every stepping entry point, like the target trace: raw [T][B][N] = uav.raw_reward of every
 * UAV after each step -- alpha * tracking + beta * boundary + gamma * duplicate of the clipped, normalised terms
 * (environment.py:211-219), BEFORE the cooperative sharing of environment.py:222-226.  The reference keeps it as a public
 * attribute of each UAV (uav.py:50).  Row t of a call's T steps at raw + t * B * N; capacity_steps >= the largest T passed
 * while the buffer is set (checked); raw = NULL switches the output off (the default). */
int uavtrack_set_raw_reward_output(uavtrack_env *env, float *raw, int32_t capacity_steps);

/* Environment.step (environment.py:120-164) for a caller that lives on the HOST, the way the reference's own training
 * loop calls it (train.py:160-185: a Python list of actions in; next_states, the reward dict and the covered count out,
 * one environment, one step at a time).  actions_host [B][N] int32 is a HOST pointer; the results are left in a
 * library-owned, page-locked host block that the kernels write directly through its device mapping (no device-to-host
 * copy call), together with a copy of the state as it stands behind the step (what Environment.step appends to
 * `position`, environment.py:150-155, and what callers read as uav.x / target.x).  `out` receives HOST pointers into that
 * block; the block is allocated once per handle, so the pointers are the same on every call and stay valid -- their
 * contents overwritten by the next uavtrack_step_host -- until uavtrack_destroy.
 * This entry point SYNCHRONISES `stream` before it returns (the one stepping call that does): it is meant for batches
 * of one or a few environments -- the drop-in adapter -- where a step is bound by the launch and the synchronisation,
 * not by the kernel.  Batched rollouts use uavtrack_step / uavtrack_step_many on device buffers. */
typedef struct uavtrack_host_step {
    const float   *obs;        /* [B][N][12] next_states                         (environment.py:144) */
    const float   *reward;     /* [B][N]     reward['rewards']                   (environment.py:158) */
    const float   *terms;      /* [3][B][N]  the three normalised terms          (environment.py:159-161) */
    const float   *raw;        /* [B][N]     uav.raw_reward                      (environment.py:219) */
    const int32_t *covered;    /* [B]        covered_targets                     (environment.py:146) */
    const uint8_t *done;       /* [B]        step_count >= horizon */
    const float   *ux, *uy, *uz, *uh;   /* [B][N] UAV poses behind the step (uz NULL in 2-D) */
    const int32_t *ua;                  /* [B][N] the actions just applied (uav.a) */
    const float   *tx, *ty, *tz, *th;   /* [B][M] target poses behind the step (tz NULL in 2-D) */
    const int32_t *step_count;          /* [B] */
} uavtrack_host_step;
int uavtrack_step_host(uavtrack_env *env, const int32_t *actions_host, uavtrack_host_step *out, void *stream);

/* MAAC-R accounting for reports: out[0] = neighbour pairs the stepping entry points have handed to the PMI network
 * since the handle was created (each unordered pair once per step).  A pair of UAVs that are each other's ONLY
 * neighbour is not among them: the softmax over a single neighbour is 1 whatever its score (uav.py:287-288), so such a
 * pair is never scored.  Synchronises `stream`. */
int uavtrack_pmi_pairs_scored(uavtrack_env *env, uint64_t *out, void *stream);

/* Measurement hook (bench.py's roofline legs): with profiling on, every kernel launch of the stepping entry points is
 * bracketed by a HIP event pair on the launch stream.  uavtrack_get_profile synchronises `stream`, adds the elapsed
 * milliseconds up per kernel class into ms[UAVTRACK_PROF_CLASSES] and the launch counts into launches[...] (either may
 * be NULL), and forgets the recorded pairs.  Off by default: no events, no cost. */
enum { UAVTRACK_PROF_ROLLOUT = 0,   /* rollout_kernel: the fused environment step(s) */
       UAVTRACK_PROF_SCORER  = 1,   /* MAAC-R: pmi_score_x6_kernel / pmi_score_kernel */
       UAVTRACK_PROF_MIX     = 2,   /* MAAC-R: pmi_mix_kernel (softmax mix + final clip) */
       UAVTRACK_PROF_EPSUMS  = 3,   /* MAAC-R: ep_reward_kernel (episode return from the per-step means) */
       UAVTRACK_PROF_CLASSES = 4 };
int uavtrack_set_profiling(uavtrack_env *env, int32_t on);
int uavtrack_get_profile(uavtrack_env *env, double *ms, int64_t *launches, void *stream);

/* Launch geometry of the step kernel, for reports: out[0] = workgroup size,
 * out[1] = envs per workgroup, out[2] = workgroups, out[3] = LDS bytes per
 * workgroup, out[4] = 1 if a compile-time-specialised (N, M) variant is used. */
int uavtrack_kernel_info(uavtrack_env *env, int64_t out[5]);

/* Geometry of the most recent rollout launch of a stepping entry point (MAAC-R picks it per launch: the single-wavefront
 * variant exists for launches with every output and no extras only): out[0] = workgroup size, out[1] = envs per
 * workgroup, out[2] = workgroups, out[3] = 1 if the single-wavefront (pooled pair-list slots) kernel variant ran.
 * All zero before the first launch. */
int uavtrack_launch_info(uavtrack_env *env, int64_t out[4]);

/* Which rollout kernel instantiation the most recent rollout launch ran, as its template arguments: out[0], out[1] = the
 * compile-time (N, M) of a specialised shape (0, 0: the generic kernel), out[2] = the reward mode AS INSTANTIATED (the
 * greedy baseline's PMI slot is the RAW kernel), out[3] = 1 for the 3-D kernel, out[4] = the policy (0 the caller's
 * actions, 1 the greedy baseline, 2 the actor), out[5] = 1 for the every-output variant, out[6] = 1 for the variant with
 * the optional extras (automatic reset, target trace, raw rewards, state copy), out[7] = 1 for the single-wavefront
 * variant.  The tuple is written down where the kernel's address is taken, so it names the kernel that ran, not the one
 * that was asked for.  Before the first launch every entry is -1 ("none yet": all zeros is a real kernel, the generic
 * planar RAW one with an output left out). */
int uavtrack_variant_info(uavtrack_env *env, int64_t out[8]);

/* ---- the learner: ActorCritic.update + both Adam steps on the device ----
 * A handle of its own, independent of any environment (one learner may serve sharded environments).  It holds the
 * shared actor FnnPolicyNet (actor_critic.py:85-98: Linear(12,H) - ReLU - Linear(H,A) - softmax), the critic
 * FnnValueNet (actor_critic.py:101-112: Linear(12,H) - ReLU - Linear(H,1)) and one torch.optim.Adam state per
 * network (actor_critic.py:128-131: defaults betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad).
 * Parameter blobs are fp32 in torch order: actor fc1.weight [H][12], fc1.bias [H], fc2.weight [A][H], fc2.bias [A],
 * then critic fc1.weight [H][12], fc1.bias [H], fc2.weight [1][H], fc2.bias [1] -- uavtrack_learner_num_params floats. */
enum uavtrack_actor_loss {
    UAVTRACK_LOSS_REFERENCE  = 0,   /* actor_critic.py:171: log_probs [n,1] * td_delta [n] broadcasts to [n,n]:
                                       actor_loss = mean_i(-log p_i) * mean_j(delta_j) */
    UAVTRACK_LOSS_PER_SAMPLE = 1    /* actor_loss = mean_i(-log p_i * delta_i) */
};

typedef struct uavtrack_learner_config {
    uint32_t struct_size;       /* = sizeof(uavtrack_learner_config), ABI check */
    int32_t  device_id;         /* HIP device ordinal */
    int32_t  hidden;            /* H in [1, 256]             (actor_critic.py:120 hidden_dim) */
    int32_t  n_actions;         /* A = na * nc in [1, 48]    (actor_critic.py:120 action_dim) */
    int32_t  loss;              /* enum uavtrack_actor_loss */
    int32_t  pad_;              /* 0 */
    int64_t  max_batch;         /* scratch for batches up to this many rows; 0 = 65536 (see uavtrack_learner_reserve) */
    double   gamma;             /* actor_critic.py:133 */
    double   actor_lr;          /* actor_critic.py:128-129 */
    double   critic_lr;         /* actor_critic.py:130-131 */
} uavtrack_learner_config;

typedef struct uavtrack_learner uavtrack_learner;   /* opaque handle */

/* Replaces ActorCritic.__init__ (actor_critic.py:118-134).  Parameters and Adam moments start at zero, step counts
 * at 0: upload the initial weights with uavtrack_learner_set_params.  Allocates everything an update needs. */
int uavtrack_learner_create(const uavtrack_learner_config *cfg, uavtrack_learner **out);
int uavtrack_learner_destroy(uavtrack_learner *learner);

/* Floats in a parameter blob (= in each Adam moment blob). */
int uavtrack_learner_num_params(uavtrack_learner *learner, int64_t *out);

/* Grows the update scratch to batches of max_batch rows (allocates; synchronises the device).  Never shrinks. */
int uavtrack_learner_reserve(uavtrack_learner *learner, int64_t max_batch);

/* actor.load_state_dict + critic.load_state_dict (actor_critic.py:198, 203) / state_dict (actor_critic.py:183-190):
 * HOST blobs of n_floats = uavtrack_learner_num_params floats in the order above.  Synchronise `stream`.  A failing
 * set leaves the previous parameters in place. */
int uavtrack_learner_set_params(uavtrack_learner *learner, const float *params, int64_t n_floats, void *stream);
int uavtrack_learner_get_params(uavtrack_learner *learner, float *params, int64_t n_floats, void *stream);

/* uavtrack_publish_actor_weights from the learner's own parameters (the actor's four tensors at the head of the blob
 * above) into `env`'s rollout actor: stream-ordered, no synchronisation, no allocation, capturable; the parameters are
 * read when the launches execute, so a graph replayed after updates publishes the weights of that moment.  Refused,
 * with nothing enqueued, if the two handles sit on different devices, or if hidden or n_actions differ from the
 * installed actor's width or from env's na*nc. */
int uavtrack_learner_publish_actor(uavtrack_learner *learner, uavtrack_env *env, void *stream);

/* actor_optimizer / critic_optimizer .load_state_dict (actor_critic.py:199, 204) / state_dict (actor_critic.py:185,
 * 189): exp_avg and exp_avg_sq as HOST blobs in parameter order, step [8] = the Adam step count of each parameter
 * tensor (same order; int64, >= 0).  Synchronise `stream`.  A failing set leaves the previous state in place. */
int uavtrack_learner_set_optimizer_state(uavtrack_learner *learner, const float *exp_avg, const float *exp_avg_sq,
                                         const int64_t *step, int64_t n_floats, void *stream);
int uavtrack_learner_get_optimizer_state(uavtrack_learner *learner, float *exp_avg, float *exp_avg_sq, int64_t *step,
                                         int64_t n_floats, void *stream);

/* Replaces ActorCritic.update (actor_critic.py:150-179) and the PrioritizedReplayBuffer.update_priorities call behind
 * it (train.py:262 -> train.py:136-138), stream-ordered: no synchronisation, no allocation, capturable into a graph.
 * Rows are gathered in the kernel from a replay ring's stores (DEVICE pointers): states / next_states [capacity][12],
 * actions [capacity] int32, rewards [capacity]; row i of the batch is slot indices[i] (int64 [n], what the buffers'
 * sample draws), or slot i when indices == NULL (then n <= capacity).  Outputs (DEVICE): actor_loss and critic_loss
 * (fp32 scalars), td_delta [n] (nullable), priorities [capacity] (nullable): |td_delta| written at the sampled slots,
 * the last occurrence of a repeated slot winning, as the reference's loop.  Both Adam steps advance their device step
 * counts, so a replayed graph keeps counting.  Returns an error, enqueuing nothing, for a null required pointer,
 * n < 1, or n above the reserved batch.  An action outside [0, A) or an index outside [0, capacity) is found on the
 * device: that update then changes nothing (parameters, moments, steps, priorities), its losses are NaN, and the next
 * uavtrack_learner_check reports it. */
int uavtrack_learner_update(uavtrack_learner *learner, int64_t n,
                            const float *states, const int32_t *actions, const float *rewards,
                            const float *next_states, int64_t capacity, const int64_t *indices,
                            float *actor_loss, float *critic_loss, float *td_delta, float *priorities, void *stream);

/* ---- importance-weighted updates ----
 * uavtrack_learner_update with one weight per batch row: weights (DEVICE fp32 [n], in BATCH order: weights[i] belongs
 * to row i of the batch, not to slot indices[i]), w_i >= 0 -- the importance-sampling weights a prioritised draw hands
 * out with its indices (uavtrack_replay_sample, uavtrack_replay_sample_annealed).  The losses become
 *   critic_loss                            = mean_i( w_i * (V(s_i) - y_i)^2 ),  y_i = r_i + gamma * V(s'_i) detached
 *   actor_loss, UAVTRACK_LOSS_PER_SAMPLE   = mean_i( -w_i * log p_i * delta_i )
 *   actor_loss, UAVTRACK_LOSS_REFERENCE    = mean_i( -w_i * log p_i ) * mean_j( w_j * delta_j )
 * The reference's broadcast loss is a double sum over pairs, (1/n^2) sum_i sum_j (-log p_i) delta_j; the importance
 * weight of the pair (i, j) is w_i * w_j, which gives the product of the two weighted means (and stays linear in the
 * weighted mean of delta, so gradient rows still add).  Every mean divides by n, the row count, as torch's
 * (w * l).mean() does -- not by sum w.  td_delta and the priorities written back stay the unweighted delta_i and
 * |delta_i|.  With every w_i = 1 each formula is uavtrack_learner_update's, and weights == NULL makes the call exactly
 * uavtrack_learner_update: a vector of ones gives the same bits.
 * A weight that is NaN, infinite or negative is found on the device like a bad action (status bit 2): the update then
 * changes nothing, its losses are NaN and the next uavtrack_learner_check counts it.  A refused draw writes NaN weights,
 * so the update behind a refused draw is refused too, with no host involvement. */
int uavtrack_learner_update_weighted(uavtrack_learner *learner, int64_t n,
                                     const float *states, const int32_t *actions, const float *rewards,
                                     const float *next_states, int64_t capacity, const int64_t *indices,
                                     const float *weights,
                                     float *actor_loss, float *critic_loss, float *td_delta, float *priorities,
                                     void *stream);

/* ---- the split update: gradient rows and an ordered apply ----
 * uavtrack_learner_update cut between "sum" and "scale + Adam", so that one update can take its batch from several
 * rings, several calls (gradient accumulation) or several processes (data parallelism) with DEFINED bits: every sum is
 * taken in a fixed order, so every participant that applies the same rows in the same order ends with the same
 * parameters, and one row applied alone gives uavtrack_learner_update's bits.
 *
 * A gradient row is uavtrack_learner_row_floats = P + 8 fp32 words on the DEVICE (P = uavtrack_learner_num_params):
 *   [0, P)      the unscaled gradient sums in parameter order (the actor's are sums of onehot(a) - p, times delta for
 *               UAVTRACK_LOSS_PER_SAMPLE; the critic's sums of V - target): what the update forms before it scales
 *   [P, P+4)    the loss sums: sum -log p, sum delta, sum -log p * delta, sum (V - target)^2
 *   P+4, P+5    n of this row, an int64 as its low and high 32 bits
 *   P+6         int32 status bits of this row: bit 0 an action outside [0, A), bit 1 an index outside [0, capacity),
 *               bit 2 an importance weight that is NaN, infinite or negative, bit 3 (value 8) a discount that is NaN,
 *               negative or above 1 (see "multi-step targets: per-row discounts"), bit 4 (value 16) a behaviour
 *               log-probability that is NaN or positive, or a ratio that is not finite (see "the clipped surrogate")
 *   P+7         int32 P, the layout tag
 * The reference's actor loss mean(-log p) * mean(delta) is linear in mean(delta), which is why the rows can be summed:
 * the apply scales the actor's sums once by the GLOBAL -mean(delta) / N.  (Averaging per-row updates or per-row loss
 * gradients is a different rule.)
 * A row of uavtrack_learner_grad_weighted has the same layout and tag; every term of its sums carries its batch row's
 * w_i (sum -w log p, sum w delta, sum -w log p delta, sum w (V - target)^2), its n is still the row count, and weighted
 * and unweighted rows may meet in one apply.
 * All four calls are stream-ordered: no synchronisation, no allocation, capturable.  Host-side errors (a null required
 * pointer, n < 1 or above the reserved batch, count outside [1, UAVTRACK_LEARNER_MAX_ROWS]) enqueue nothing. */
#define UAVTRACK_LEARNER_MAX_ROWS 64   /* rows one apply takes: ranks x micro-batches */

/* Words of a gradient row (P + 8). */
int uavtrack_learner_row_floats(uavtrack_learner *learner, int64_t *out);

/* The forwards, the backwards and the sums of uavtrack_learner_update on one batch (same arguments), into `row`
 * (DEVICE, row_floats words).  td_delta [n] is required.  Changes no learner state except scratch: parameters, moments,
 * steps and the verdict of the last apply stay.  Bad actions or indices are recorded in the row. */
int uavtrack_learner_grad(uavtrack_learner *learner, int64_t n,
                          const float *states, const int32_t *actions, const float *rewards,
                          const float *next_states, int64_t capacity, const int64_t *indices,
                          float *td_delta, float *row, void *stream);

/* uavtrack_learner_grad with importance weights (DEVICE fp32 [n], batch order; see "importance-weighted updates"):
 * weights == NULL makes it exactly uavtrack_learner_grad.  td_delta stays the unweighted delta. */
int uavtrack_learner_grad_weighted(uavtrack_learner *learner, int64_t n,
                                   const float *states, const int32_t *actions, const float *rewards,
                                   const float *next_states, int64_t capacity, const int64_t *indices,
                                   const float *weights, float *td_delta, float *row, void *stream);

/* One update from rows [count][row_floats] (DEVICE): gradient and loss sums added in row order in fp32, N = sum of the
 * rows' n, losses and scales as uavtrack_learner_update forms them from N, then both Adam steps and the step counts.
 * If any row carries a status bit or another layout tag, the apply changes nothing (parameters, moments, steps), its
 * losses are NaN and the next uavtrack_learner_check counts it: exactly a refused update.  The verdict stays on the
 * handle for uavtrack_learner_write_priorities. */
int uavtrack_learner_apply(uavtrack_learner *learner, const float *rows, int64_t count,
                           float *actor_loss, float *critic_loss, void *stream);

/* The priority write of uavtrack_learner_update for one row's batch: |td_delta[i]| into priorities[indices[i]]
 * (indices == NULL: slot i), the last occurrence of a repeated slot winning.  Writes nothing if the most recent apply
 * (or update) on this handle was refused, so a refused update leaves every participant's priorities alone. */
int uavtrack_learner_write_priorities(uavtrack_learner *learner, int64_t n, const int64_t *indices, int64_t capacity,
                                      const float *td_delta, float *priorities, void *stream);

/* ---- regularisation: an entropy bonus and gradient-norm clipping (both off by default) ----
 * Two optional settings of a learner handle.  With both at their defaults every call above enqueues exactly the kernels
 * it enqueued without them, with the same arguments.
 *
 * Entropy bonus c >= 0 (entropy_coef), UAVTRACK_LOSS_PER_SAMPLE only.  With p_i = softmax(z_i) and
 * H_i = -sum_o p_io log p_io the actor loss becomes
 *   actor_loss = mean_i( w_i * ( -log p_i(a_i) * delta_i - c * H_i ) )       (w_i = 1 without weights; the mean divides by n)
 * The accumulated logit weight of a batch row is w_i * ( delta_i * (onehot - p_i)_o - c * p_io * (log p_io + H_i) ),
 * still scaled by -1 / N in the Adam step, so a gradient row keeps its P + 8 words and its tag, and regularised rows add
 * up in an apply like any others: the entropy term is one more summand of the same per-row sums.  actor_loss is the whole
 * loss above; loss word [P+2] of a row carries sum w_i (-log p_i delta_i - c H_i), words [P], [P+1], [P+3] are unchanged.
 * Every log p of a regularised row comes from the logits, (z_o - max) - log sum exp(z - max), so H_i and its gradient are
 * finite for every finite logit vector, also where a small probability underflows to 0 in fp32 (such an action adds 0).
 * The reference form scales the actor's gradient sums ONCE by the global -mean(delta) / N after they are added; an
 * entropy term would need a scale of its own (-1 / N), that is a second actor block in the row: c != 0 on a
 * UAVTRACK_LOSS_REFERENCE learner is refused.  With c == 0 the row loop computes what it computed before, to the bit.
 *
 * Gradient-norm clipping, one max_norm per network (actor, critic), each > 0 or +inf for off:
 * torch.nn.utils.clip_grad_norm_(net.parameters(), max_norm).  g is the scaled gradient the Adam step forms (the ordered
 * sum over workgroup partials or rows, times the network's scale); norm = sqrt(sum_p g_p^2) over that network's
 * parameters; coef = min(1, max_norm / (norm + 1e-6)); Adam sees coef * g.  The sum of squares is taken in fp64 in a
 * fixed order, coef is formed in double and rounded to fp32 once, so every participant of a split or data-parallel
 * update gets the same coef bits from the same rows; norm + 1e-6 <= max_norm gives coef == 1.0f exactly, and an update
 * that does not clip is bit for bit the unclipped one.  A non-finite norm propagates as torch's default does (nothing
 * new is refused); a refused update stays a no-op.  Clipping applies to update, update_weighted and apply alike, in both
 * loss forms; in an apply the norm is that of the summed rows.  With both max norms +inf no additional kernel is launched;
 * otherwise an update adds two small launches and one more pass over P floats.
 *
 * Gradient rows carry no settings: every learner that takes part in one update (ranks, shards) must be given the same. */

/* Host-side settings, read when a later update / grad / apply is ENQUEUED (a captured graph keeps the values it was
 * captured with, as it keeps beta).  entropy_coef >= 0 finite; max norms > 0 or +inf.  Refused, changing nothing:
 * NaN / negative / zero-norm values; entropy_coef != 0 on a UAVTRACK_LOSS_REFERENCE learner (see above). */
int uavtrack_learner_set_regularisation(uavtrack_learner *learner, double entropy_coef, double actor_max_norm,
                                        double critic_max_norm);
/* out = {entropy_coef, actor_max_norm, critic_max_norm} as they were last set ({0, +inf, +inf} at create). */
int uavtrack_learner_get_regularisation(uavtrack_learner *learner, double out[3]);

/* Optional diagnostics, caller-owned DEVICE buffers (not copied; NULL uninstalls either).  Installing them changes no
 * other output bit.
 *   entropy   fp32 [capacity_rows]: H_i of batch row i, written by every update or grad while installed, whatever c is;
 *             0 for a batch row that was not used (bad action, index or weight).  An update or grad of more rows than
 *             capacity_rows while entropy is installed is refused on the host, enqueuing nothing.
 *   grad_norm fp32 [2]: the actor's and the critic's gradient norm before clipping, written by every update or apply
 *             that clips (at least one finite max norm; a huge finite one observes without clipping), NaN for a refused one. */
int uavtrack_learner_set_diagnostics(uavtrack_learner *learner, float *entropy, int64_t capacity_rows, float *grad_norm);

/* ---- multi-step targets: per-row discounts ----
 * The target of batch row i becomes
 *   y_i = r_i + d_i * V(s'_i),   d_i = discounts[slot of row i],   delta_i = y_i - V(s_i)
 * discounts is a DEVICE fp32 [capacity] store, indexed by SLOT and gathered through the same index vector as the reward
 * (slot indices[i], or slot i without indices) -- unlike the importance weights, which are in batch order.  It is the
 * fifth store of an n-step ring (uavtrack_replay_add_rollout_nstep leaves gamma^m there, m the transition's horizon), but
 * any per-slot factor in [0, 1] will do: d_i = 0 means "do not bootstrap", which a caller can use to mark a true terminal
 * state.  Everything downstream of delta and y is unchanged: both loss forms, the weights, the entropy term, clipping,
 * td_delta and the priorities.  discounts == NULL means d_i = (float)gamma of the learner's config, the expression of
 * uavtrack_learner_update, and a store filled with (float)gamma gives the same bits.  weights and discounts are each
 * nullable; with both NULL the two calls below are exactly uavtrack_learner_update and uavtrack_learner_grad.
 * A d_i that is NaN, negative or above 1 is found on the device like a bad action: status bit 3 (value 8) in the status
 * word and in word P + 6 of a gradient row; the update or apply then changes nothing, its losses are NaN, the next
 * uavtrack_learner_check counts it, and uavtrack_learner_write_priorities stays gated on that verdict.  A gradient row
 * keeps its P + 8 words and its tag, and rows with and without discounts may meet in one apply.  Host-side errors are
 * those of uavtrack_learner_update_weighted / _grad_weighted. */
int uavtrack_learner_update_discounted(uavtrack_learner *learner, int64_t n,
                                       const float *states, const int32_t *actions, const float *rewards,
                                       const float *next_states, int64_t capacity, const int64_t *indices,
                                       const float *weights, const float *discounts,
                                       float *actor_loss, float *critic_loss, float *td_delta, float *priorities,
                                       void *stream);
int uavtrack_learner_grad_discounted(uavtrack_learner *learner, int64_t n,
                                     const float *states, const int32_t *actions, const float *rewards,
                                     const float *next_states, int64_t capacity, const int64_t *indices,
                                     const float *weights, const float *discounts, float *td_delta, float *row,
                                     void *stream);

/* ---- the critic alone: V(x) outside an update ----
 * values[i] = V(rows[i]) for n rows x[12] (DEVICE fp32 [n][12], 16-byte aligned; values DEVICE fp32 [n]) with the
 * learner's critic parameters, by exactly the chain of the update's own V(s), H = hidden:
 *   p_j = b1c[j]; for k = 0 .. 11: p_j = fmaf(W1c[j][k], x[k], p_j); h_j = fmaxf(p_j, 0);
 *   z = b2c[0];   for j = 0 .. H - 1: z = fmaf(W2c[j], h_j, z);      V = z
 * so a caller reads, bit for bit, the V(s) an update with the same parameters forms.  Stream-ordered, no
 * synchronisation, no allocation, capturable; it needs no scratch, so n is not limited by the reserved batch, and it
 * changes no learner state.  The parameters are read when the launch executes: a graph replayed after updates evaluates
 * the critic of that moment.  Returns an error, enqueuing nothing, for a null pointer, n < 1 or misaligned rows. */
int uavtrack_learner_values(uavtrack_learner *learner, int64_t n, const float *rows, float *values, void *stream);

/* ---- the target critic: bootstrap from a second copy of the critic, synced softly or periodically (off by default) ----
 * A learner may hold a second copy of the critic's parameters, the target theta-: 14 H + 1 fp32 words in the critic's own
 * torch order, fc1.weight [H][12], fc1.bias [H], fc2.weight [1][H], fc2.bias [1].  With it off, every call above enqueues
 * exactly the kernels it enqueued without it.  While a target is enabled:
 *
 * Bootstrap.  y_i = r_i + d_i * V_target(s'_i), with theta- as it stands when the gradient kernel executes;
 * delta_i = y_i - V(s_i).  V(s_i), both backward passes, the losses, td_delta and the priorities are formed as before, in
 * both loss forms, with weights, per-row discounts, truncated ratios, the entropy bonus and clipping: none of them
 * touches V(s').  V_target(s') is the chain of uavtrack_learner_values (layer 1 in k order, layer 2 in j order, explicit
 * fmaf) over theta-, so while theta- holds the critic's bits an update forms the bits of the update without a target.
 * This holds for update, update_weighted, update_discounted and the three grad calls alike.
 *
 * Sync rule.  Once per SUCCESSFUL update or apply, behind its Adam step on the same stream and gated on the same status
 * word: a refused update or apply leaves theta- untouched.  w is the critic just stepped, t the target, word by word:
 *   UAVTRACK_TARGET_POLYAK, tau in (0, 1]:  tau32 = (float)tau and omt = 1.0f - tau32, both formed once on the host;
 *       t <- fl( fl(omt * t) + fl(tau32 * w) )
 *     two fp32 multiplies and one fp32 add, each rounded to nearest on its own, never contracted into an FMA: a float32
 *     mirror that performs the three operations reproduces every bit.  At tau = 1, omt = 0 and t <- w: the critic's bits
 *     (for finite t; a word w = -0.0f comes out as +0.0f where omt * t is +0).
 *   UAVTRACK_TARGET_PERIODIC, period >= 1:  t <- w if step % period == 0, where step is the critic's fc1.weight Adam
 *     step count on the device (step[4] of uavtrack_learner_get_optimizer_state) AFTER this update advanced it.  The
 *     counter lives on the device: a replayed graph keeps the schedule, and so does a learner resumed from a checkpoint.
 * The split update: uavtrack_learner_grad* bootstraps from theta-, uavtrack_learner_apply runs the sync rule behind its
 * Adam step.  Gradient rows keep their P + 8 words and carry no settings: the participants of one update must hold
 * equal settings and equal theta-; they then stay bitwise equal, each running the same rule on the same bits.
 *
 * What is promised bitwise: the arithmetic above; that an update whose theta- equals the critic's bits is the update
 * without a target; that a learner that disabled its target again updates like one that never had one.  Nothing is
 * claimed about learning curves.  Cost on one MI355X: DESIGN.md section 9. */
enum uavtrack_target_mode {
    UAVTRACK_TARGET_OFF      = 0,   /* bootstrap from the online critic (the default) */
    UAVTRACK_TARGET_POLYAK   = 1,   /* soft sync by tau after every successful update */
    UAVTRACK_TARGET_PERIODIC = 2    /* hard copy whenever the device step count is a multiple of period */
};

/* Host-side settings, read when a later update / grad / apply is ENQUEUED (a captured graph keeps the ones it was
 * captured with).  mode: enum uavtrack_target_mode; tau is read for _POLYAK only, period for _PERIODIC only.
 * OFF -> on allocates the block (once; it is kept for the handle's life, so this call is not for use inside a capture)
 * and hard-copies the current critic into it, ordered on `stream`.  Changing tau, period or the mode while a target is
 * enabled keeps theta-.  _OFF returns the bootstrap to the online critic; enabling again hard-copies again.
 * Refused, changing nothing: an unknown mode, tau outside (0, 1] or NaN, period < 1. */
int uavtrack_learner_set_target(uavtrack_learner *learner, int32_t mode, double tau, int64_t period, void *stream);
/* out = {mode, tau as it was set (0 unless _POLYAK), period (0 unless _PERIODIC)}; {0, 0, 0} at create. */
int uavtrack_learner_get_target(uavtrack_learner *learner, double out[3]);
/* theta- <- the critic as it stands when the copy executes: stream-ordered, no synchronisation, no allocation,
 * capturable.  An error while no target is enabled. */
int uavtrack_learner_sync_target(uavtrack_learner *learner, void *stream);
/* theta- as a HOST blob of n_floats = 14 H + 1 floats in the order above.  Synchronise `stream`, like
 * uavtrack_learner_set_params.  An error while no target is enabled. */
int uavtrack_learner_set_target_params(uavtrack_learner *learner, const float *params, int64_t n_floats, void *stream);
int uavtrack_learner_get_target_params(uavtrack_learner *learner, float *params, int64_t n_floats, void *stream);
/* uavtrack_learner_values with theta- in the critic's place: the same kernel, chain and argument rules, theta- read when
 * the launch executes.  An error while no target is enabled. */
int uavtrack_learner_values_target(uavtrack_learner *learner, int64_t n, const float *rows, float *values, void *stream);

/* ---- the actor alone, and off-policy correction: truncated importance ratios as update weights ----
 * Rows of a replay ring were acted by the actor of the moment they were added (the behaviour policy mu), not by the one
 * an update differentiates (pi).  The truncated ratio rho_i = min(rho_bar, pi(a_i|s_i) / mu(a_i|s_i)) is one weight per
 * batch row, and the weighted entry points above take one weight per batch row: with w_i = rho_i,
 * UAVTRACK_LOSS_PER_SAMPLE trains mean_i(-rho_i log p_i delta_i) and mean_i(rho_i (V(s_i) - y_i)^2), rho a constant of
 * the differentiation -- the truncated-importance-sampling policy gradient and the rho-weighted TD(0) critic, the
 * one-step case of V-trace.  The ratio corrects the FIRST action of a transition only: on an n-step or lambda ring the
 * later actions of the window stay uncorrected (no traces; Retrace and full V-trace are not built).
 *
 * log pi(a|s) of a row, with the learner's actor parameters as they stand when the launch executes, H = hidden:
 *   p_j = b1a[j]; for k = 0 .. 11: p_j = fmaf(W1a[j][k], s[k], p_j); h_j = fmaxf(p_j, 0);
 *   z_o = b2a[o]; for j = 0 .. H - 1: z_o = fmaf(W2a[o][j], h_j, z_o);
 *   log p_a = (z_a - max_o z_o) - logf(sum_o expf(z_o - max)),   the sum in ascending o
 * the chains of the update's own actor forward and the logits form of its regularised rows: finite for every finite
 * logit vector, also where a probability underflows.  The bits of a row depend on the row and the parameters alone, not
 * on n, on the addressing mode or on where in a launch the row falls.  A slot outside [0, capacity) or an action outside
 * [0, A) gives NaN for that row; no status word is involved.
 * All three calls are stream-ordered: no synchronisation, no allocation, no scratch (n is not limited by the reserved
 * batch), capturable, and they change no learner state.  states (DEVICE fp32 [capacity][12], 16-byte aligned) and
 * actions (DEVICE int32 [capacity]) are a ring's stores.  Returns an error, enqueuing nothing, for a null required
 * pointer, n < 1, n > capacity where no indices choose the rows, misaligned states, and what each call names below. */

/* batch order: row i reads slot indices[i] (indices NULL: slot i, capacity >= n); log_probs[i] (DEVICE fp32 [n]) */
int uavtrack_learner_log_probs(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                               int64_t capacity, const int64_t *indices, float *log_probs, void *stream);

/* ring window: slots (first + k) % capacity, k < n <= capacity, 0 <= first < capacity; writes log_mu[slot] (DEVICE fp32
 * [capacity], a ring's sixth store).  Run behind a ring add over the window the add has just written, it leaves the
 * behaviour log-probabilities of the new transitions -- provided the learner's actor is, at that moment, the one that
 * acted: the add has to come before the updates of the iteration.  (A rollout whose actor runs on the f16 matrix cores
 * "at fp32 accuracy" sampled from this distribution to that accuracy, not to the bit.) */
int uavtrack_learner_log_probs_window(uavtrack_learner *learner, const float *states, const int32_t *actions,
                                      int64_t capacity, int64_t first, int64_t n, float *log_mu, void *stream);

/* The weights of a batch, fused with the forward.  With src_i = indices[i] (indices NULL: i):
 *   rho_i          = fminf((float)rho_bar, expf(log p_i - log_mu[src_i]))
 *   weights_out[i] = (weights_in ? weights_in[i] : 1.0f) * rho_i       (DEVICE fp32 [n]; weights_out may alias weights_in)
 *   rho_out[i]     = rho_i                                              (DEVICE fp32 [n], nullable)
 * log_mu is DEVICE fp32 [capacity], indexed by slot.  rho_bar > 0; +inf means untruncated (rho_bar <= 0 or NaN is
 * refused on the host).  A log_mu that is NaN ("unknown") or > 0 gives rho_i = NaN, and so do a bad slot and a bad
 * action; an overflowing untruncated ratio is +inf.  The update behind the call refuses a NaN, infinite or negative
 * weight on the device (status bit 2), so an unknown behaviour policy refuses the update with no host involvement.
 * expf(0.0f) == 1.0f: a row whose log_mu holds the bits this kernel would form now has rho_i == 1 exactly, so an
 * on-policy batch at rho_bar >= 1 trains with the bits of the unweighted update.  weights_in carries a prioritised
 * draw's importance weights; the product is not normalised again.
 * Measured on one MI355X, H = 128, A = 12: uavtrack_learner_log_probs_window over 2 048 000 slots
 * 212 us and over 16 384 000 slots 1.60 ms (2.3 x uavtrack_learner_values on the same rows; bound by the LDS reads of the
 * actor's records); this call at n = 65 536 28 us; an update of 65 536 rows behind a draw 863 us with it against 829 us
 * without (uniform ring), 1 737 us against 1 707 us (prioritised ring with importance weights). */
int uavtrack_learner_ratio_weights(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                   const float *log_mu, int64_t capacity, const int64_t *indices, double rho_bar,
                                   const float *weights_in, float *weights_out, float *rho_out, void *stream);

/* ---- the clipped surrogate: PPO's actor loss from stored behaviour log-probabilities (UAVTRACK_LOSS_PER_SAMPLE only) ----
 * The other standard answer to rows an older actor acted: differentiate THROUGH the ratio r = pi / mu and stop a row's
 * policy gradient once r has left [1 - eps, 1 + eps] in the direction its advantage pushes.  Batch row i reads slot
 * src_i (indices[i], or i); w_i is its weight (1 without weights), c the entropy coefficient, A_i = delta_i the TD error
 * of the update (a constant of the differentiation).  eps32 = (float)clip_eps, lo = 1.0f - eps32, hi = 1.0f + eps32,
 * both folded on the host (hi = +inf for clip_eps = +inf):
 *   lp_i   = (z_a - max_o z_o) - logf(sum_o expf(z_o - max))      the bits uavtrack_learner_log_probs forms for the row
 *   r_i    = expf(lp_i - log_mu[src_i])
 *   pass_i = (A_i >= 0) ? (r_i <= hi) : (r_i >= lo)               inclusive: a ratio on the boundary still passes
 *   surr_i = pass_i ? r_i * A_i : ((A_i >= 0) ? hi : lo) * A_i    = min(r A, clip(r, lo, hi) A)
 *   actor_loss   = mean_i( w_i * ( -surr_i - c * H_i ) )
 *   logit weight = w_i * ( (pass_i ? r_i * A_i : 0) * (onehot - p_i)_o - c * p_io * (log p_io + H_i) ),  scaled by -1 / N
 * The critic, td_delta, the priorities, per-row discounts, the target critic, gradient-norm clipping and the entropy term
 * are what they are without it.  Loss words [P], [P+1], [P+3] of a gradient row keep their meaning and word [P+2] carries
 * sum w_i (-surr_i - c H_i); a row keeps its P + 8 words and its tag, so rows with and without the clipped loss may meet
 * in one apply (rows carry no settings: participants of one update pass equal clip_eps).  log p, p and H of a clipped
 * row always come from the logits.  The products are ordered (A_i * r_i) first, so r_i == 1.0f with pass_i true leaves
 * the bits of the per-sample weight: a batch whose log_mu holds the bits uavtrack_learner_log_probs forms now
 * (expf(0.0f) == 1.0f) trains, at any clip_eps >= 0, with the parameters, moments, td_delta, critic loss and priorities
 * of the per-sample update; its actor_loss is mean(-w (A + c H)), not mean(w (-log p A - c H)).
 * The reference form scales the actor's sums ONCE by the global -mean(delta) / N, and a per-row gate cannot share that
 * scale: a UAVTRACK_LOSS_REFERENCE learner is refused on the host.
 * log_mu is DEVICE fp32 [capacity], indexed by SLOT and gathered beside the reward (a behaviour ring's sixth store).
 * ratio_out (DEVICE fp32 [n], nullable, batch order) receives r_i whatever clip_eps is, NaN for a row that set a status
 * bit: the clip fraction mean(|r - 1| > eps) and the approximate KL mean(-log r) are one reduction over it.
 * Refusals, found on the device like a bad action: a drawn slot whose log_mu is NaN ("unknown") or > 0, or whose r_i is
 * not finite, sets status bit 4 (value 16) in the status word and in word P + 6 of a row, and that row is not used; the
 * update or apply then changes nothing, its losses are NaN, the next uavtrack_learner_check counts it, and
 * uavtrack_learner_write_priorities stays gated on that verdict.
 * Both calls are stream-ordered: no synchronisation, no allocation, capturable.  Host-side errors, enqueuing nothing:
 * those of uavtrack_learner_update_discounted / _grad_discounted, a null log_mu, clip_eps NaN or negative (+inf is
 * allowed and never clips), a UAVTRACK_LOSS_REFERENCE learner.  weights and discounts are each nullable.
 * No second actor forward runs: the gradient kernel has the logits already.  Cost on one MI355X: DESIGN.md section 9. */
int uavtrack_learner_update_clipped(uavtrack_learner *learner, int64_t n,
                                    const float *states, const int32_t *actions, const float *rewards,
                                    const float *next_states, int64_t capacity, const int64_t *indices,
                                    const float *weights, const float *discounts,
                                    const float *log_mu, double clip_eps, float *ratio_out,
                                    float *actor_loss, float *critic_loss, float *td_delta, float *priorities,
                                    void *stream);
int uavtrack_learner_grad_clipped(uavtrack_learner *learner, int64_t n,
                                  const float *states, const int32_t *actions, const float *rewards,
                                  const float *next_states, int64_t capacity, const int64_t *indices,
                                  const float *weights, const float *discounts,
                                  const float *log_mu, double clip_eps, float *ratio_out,
                                  float *td_delta, float *row, void *stream);

/* ---- batch-normalised advantages for the per-sample losses (UAVTRACK_LOSS_PER_SAMPLE only; off by default) ----
 * Without it the advantage that multiplies grad log p is the raw TD error delta_i.  This setting standardises it,
 *   A_i = fl( fl(delta_i - mean32) * inv32 )        two fp32 operations, each rounded to nearest on its own,
 * with (mean32, inv32) the mean and the reciprocal standard deviation of the batch's own delta (UAVTRACK_ADVANTAGE_BATCH)
 * or a pair the caller keeps in device memory (UAVTRACK_ADVANTAGE_GIVEN).  A_i replaces delta_i wherever delta_i is the
 * actor's ADVANTAGE: the logit weight, the actor-loss term -log p_i A_i, and under the clipped surrogate the gate
 * (pass_i = A_i >= 0 ? r_i <= hi : r_i >= lo), r_i A_i and surr_i.  Everything else keeps the raw delta_i: the critic's
 * value weight and loss, td_delta, loss word [P+1] (sum w delta) and the priorities.  Importance weights and truncated
 * ratios multiply afterwards, as before (the statistics are unweighted, over the rows of the batch); the entropy term is
 * additive and unchanged.  A gradient row keeps its P + 8 words and its tag; normalised and raw rows may meet in one
 * apply.  Rows carry no settings, and every row is standardised by the statistics of ITS OWN batch: a split update is K
 * independently standardised draws (as each draw's importance weights are normalised by its own maximum), and its
 * participants must hold equal settings.  The setting acts on every update and grad entry point (plain, _weighted,
 * _discounted, _clipped), whose signatures are unchanged.  With the mode RAW every call enqueues exactly what it enqueued
 * before, with the same arguments.
 *
 * UAVTRACK_ADVANTAGE_BATCH, for a batch of n >= 2 rows, three steps ahead of the gradient kernel on the same stream:
 *  1. TD pass.  delta_i = (r_i + d_i V'(s'_i)) - V(s_i) of every row into library scratch: V' the target critic while one
 *     is enabled, d_i the discount store's or (float)gamma; the chains of uavtrack_learner_values and the target as one
 *     multiply and one add, each rounded on its own.  These are the bits the gradient kernel forms for the row (and
 *     leaves in td_delta).  A row whose index is out of range counts as 0 (the update is refused anyway).
 *  2. Statistics in fp64 from the fp32 delta_i, in a fixed order that does not depend on the launch geometry: rows in
 *     chunks of 256 consecutive rows (chunk c = rows [256 c, 256 c + 256), the last chunk padded with zeros that are not
 *     counted in n); inside a chunk the halving tree x[k] += x[k + h] for h = 128, 64 .. 1 (k < h) over the 256 terms in
 *     row order; the chunk sums added in ascending chunk order, starting from 0.
 *       S = sum delta_i,  mean64 = S / n;   Q = sum (delta_i - mean64)^2, the difference, the product and the adds as
 *       separate fp64 operations;   std64 = sqrt(Q / (n - 1))  (the unbiased form of torch.Tensor.std());
 *       inv64 = 1 / (std64 + eps),  eps a double, 1e-8 by default.
 *     stats = {(float)mean64, (float)inv64, (float)std64}: three floats of DEVICE memory, the handle's own or a buffer
 *     the caller installed (uavtrack_learner_set_advantage_stats), written by every batch-mode update or grad.
 *  3. The gradient kernel reads mean32 = stats[0], inv32 = stats[1] and forms A_i as above.
 * Every delta_i equal gives std64 = 0, inv32 = (float)(1 / eps) and A_i = 0 exactly: the actor does not move.
 * The scratch (n floats and two doubles per chunk) is allocated when the mode BATCH is first set, at the reserved batch
 * size, and grown by uavtrack_learner_reserve; no update, grad or apply allocates or synchronises, and all of them stay
 * capturable.  Batch mode adds four small launches to an update or grad (TD pass, squares, statistics, and one behind the
 * gradient kernel that turns stats into NaN where the call was refused).
 *
 * UAVTRACK_ADVANTAGE_GIVEN: no TD pass; the gradient kernel reads {mean32, inv32} from `given`, a caller-owned DEVICE
 * fp32 [2] that is not copied and is read when the launch executes (like the entropy buffer): running statistics, or
 * statistics a caller has reduced over shards or ranks.  {0.0f, 1.0f} leaves every bit of the RAW update of a learner
 * whose entropy diagnostics are installed or entropy_coef != 0 (x - 0 and x * 1 are exact; the kernel is the regularised
 * body), and the parameters, moments, losses, td_delta and priorities of any RAW update.
 *
 * Refusals.  On the host, enqueuing nothing: (set) an unknown mode, eps NaN or negative, GIVEN with given == NULL, a mode
 * other than RAW on a UAVTRACK_LOSS_REFERENCE learner -- that form scales the actor's gradient sums once by the global
 * -mean(delta) / N, and a standardised advantage has mean 0; (update / grad) n < 2 in BATCH mode.  On the device, like a
 * bad action: a mean32 that is not finite or an inv32 that is NaN, infinite or negative sets status bit 6 (value 64) in
 * the status word and in word P + 6 of a row; the update or apply changes nothing, its losses are NaN and the next
 * uavtrack_learner_check counts it.  (In BATCH mode that is a batch whose delta is not finite.)  An update refused on the
 * device for any reason behaves as before and leaves NaN in all three stats words.
 * Not part of checkpoints, and not carried by sharding's learner state, like the regularisation settings.
 * Cost on one MI355X: DESIGN.md section 9. */
enum uavtrack_advantage_mode {
    UAVTRACK_ADVANTAGE_RAW   = 0,   /* A_i = delta_i (the default) */
    UAVTRACK_ADVANTAGE_BATCH = 1,   /* standardised by the batch's own mean and standard deviation */
    UAVTRACK_ADVANTAGE_GIVEN = 2    /* standardised by the caller's {mean, inv_std} in device memory */
};

/* Host-side settings, read when a later update / grad is ENQUEUED (a captured graph keeps what it was captured with).
 * eps is read in BATCH mode, given in GIVEN mode (ignored otherwise; eps must still be >= 0).  The first BATCH allocates
 * the TD scratch (not for use inside a capture).  A refused call changes nothing. */
int uavtrack_learner_set_advantage(uavtrack_learner *learner, int32_t mode, double eps, const float *given);
/* mode, eps and given as they were last set ({RAW, 1e-8, NULL} at create). */
int uavtrack_learner_get_advantage(uavtrack_learner *learner, int32_t *mode, double *eps, const float **given);
/* Where BATCH mode leaves {mean, inv_std, std}: a caller-owned DEVICE fp32 [3] (not copied, in the style of
 * uavtrack_learner_set_diagnostics; it must outlive the updates enqueued while it is installed), or NULL for three
 * floats inside the handle, the default.  Host-side, read at enqueue; the gradient kernel reads the pair from there. */
int uavtrack_learner_set_advantage_stats(uavtrack_learner *learner, float *stats);

/* ---- stored advantages: the actor's advantage from a per-slot store (UAVTRACK_LOSS_PER_SAMPLE only) ----
 * uavtrack_learner_update_clipped / _grad_clipped with one more array, advantages: DEVICE fp32 [capacity], indexed by SLOT
 * and gathered beside the reward (a GAE ring's seventh store, uavtrack_replay_add_rollout_gae); log_mu is NULLABLE here
 * (NULL: no clipped surrogate; clip_eps and ratio_out are then not read).
 * Wherever the actor uses an advantage -- the logit weight, the actor-loss term, and under the clipped surrogate the gate,
 * r_i A_i and surr_i -- x_i = advantages[src_i] takes the place of delta_i, with the advantage mode applied on top:
 *     A_i = fl( fl(x_i - mean32) * inv32 )
 *   RAW    the same kernels with the handle's constant pair {0.0f, 1.0f}: x - 0 and x * 1 are exact, A_i = x_i;
 *   GIVEN  the caller's pair;
 *   BATCH  a small gather kernel writes x_i (0 for an index out of range) into the TD scratch in the TD pass's place;
 *          steps 2 and 3 above then run unchanged over it, so the order stated there describes these statistics too.
 * Everything else keeps delta_i = (r_i + d_i V'(s'_i)) - V(s_i) as it is: the critic's value weight and loss, td_delta,
 * loss word [P+1] and the priorities.  With the GAE ring's reward = G_t and discount = +0 the critic regresses on the fixed
 * value target and the actor follows the fixed advantage: both constants of the iteration.  A store that holds the bits of
 * td_delta of the plain per-sample update of the same batch leaves that update's parameters, moments, td_delta, critic
 * loss and priorities.
 * The four kernels are further instantiations of the gradient body (always with the entropy and advantage blocks), chosen
 * by (target critic on, log_mu given) from a table of their own; the other entry points launch what they launched.
 * A gradient row keeps its P + 8 words and its tag, so stored and plain rows may meet in one apply.
 * Refusals.  On the host, enqueuing nothing: those of the _clipped forms (log_mu == NULL is allowed), a null advantages, a
 * UAVTRACK_LOSS_REFERENCE learner (that form scales the actor's sums once by -mean(delta) / N, a factor a per-row
 * advantage cannot share).  On the device, like a bad action: a drawn slot whose advantage is NaN ("unknown") or infinite
 * sets status bit 7 (value 128) in the status word and in word P + 6 of a row, and that row is not used; the update or
 * apply then changes nothing, its losses are NaN and the next uavtrack_learner_check counts it.
 * Stream-ordered: no synchronisation, no allocation, capturable.  Cost on one MI355X: DESIGN.md section 9. */
int uavtrack_learner_update_stored(uavtrack_learner *learner, int64_t n,
                                   const float *states, const int32_t *actions, const float *rewards,
                                   const float *next_states, int64_t capacity, const int64_t *indices,
                                   const float *weights, const float *discounts, const float *advantages,
                                   const float *log_mu, double clip_eps, float *ratio_out,
                                   float *actor_loss, float *critic_loss, float *td_delta, float *priorities,
                                   void *stream);
int uavtrack_learner_grad_stored(uavtrack_learner *learner, int64_t n,
                                 const float *states, const int32_t *actions, const float *rewards,
                                 const float *next_states, int64_t capacity, const int64_t *indices,
                                 const float *weights, const float *discounts, const float *advantages,
                                 const float *log_mu, double clip_eps, float *ratio_out,
                                 float *td_delta, float *row, void *stream);

/* ---- KL early stopping for PPO epochs, latched on the device (UAVTRACK_LOSS_PER_SAMPLE only; off by default) ----
 * PPO's usual safeguard, `if approx_kl > limit: break`, for a loop that issues no host synchronisation and for a captured
 * graph that cannot break: a stop is a refusal that is not an error and that stays in force until it is reset.
 * While the stop is on, every closed clipped update (uavtrack_learner_update_clipped, or _update_stored with a log_mu)
 * evaluates the KL estimate of ITS OWN minibatch under the policy as it stands before that minibatch's step, and steps
 * only where the estimate does not exceed the limit:
 *   k_i = (r_i - 1) - log r_i    r_i the fp32 ratio the gradient kernel formed for batch row i (what ratio_out receives),
 *                                widened to fp64; two fp64 subtractions and an fp64 log, as written.  k_i >= 0;
 *                                r_i == 1.0f gives exactly 0; an underflowed r_i == 0 gives +inf, which stops.
 *   kl  = (float)( S / n )       S = sum k_i in fp64 in the order of the advantage statistics above: rows in chunks of 256
 *                                consecutive rows, the last padded with zeros; inside a chunk the halving tree
 *                                x[k] += x[k + h], h = 128 .. 1; chunk sums added in ascending chunk order from 0.0.
 * The statistic is unweighted: importance weights do not enter it.  kl_out[0] receives kl.  Where kl > (float)limit,
 * compared in fp32, the latch state[0] is set and this update is STOPPED; while the latch is set every later update on
 * this learner is stopped too, whatever its own KL would be, until uavtrack_learner_kl_reset.  limit = +inf observes and
 * never stops.  state = {stopped (0 or 1), skipped}: skipped counts the stopped updates since the last reset, the one that
 * tripped the latch included.
 * A stopped update sets status bit 8 (value 256) in the status word and nothing else: both Adam steps and the step
 * counters, the target critic's sync and the priority write are skipped as for a refused update, and its losses are NaN;
 * but it is NOT a refusal, and uavtrack_learner_check does not count it.  The update that trips the latch has run its
 * gradient kernel: td_delta, ratio_out and the entropy buffer hold its rows.  An update that meets the latch set returns
 * from the gradient kernel before the first tile: it writes neither td_delta, ratio_out nor entropy, inspects no input
 * (so it cannot be refused), and leaves kl_out at the last evaluated value.  After either, the advantage statistics of
 * BATCH mode are NaN and grad_norm is NaN, as after a refused update: BATCH mode's statistics pass runs ahead of the
 * gradient kernel as before (and still reads the rows), and while the stop is on its seal runs behind the KL pass's
 * verdict.  An update refused on the device never sets the latch, and leaves kl_out NaN.
 * A sweep's cursor and a ring's draw counter are advanced by the DRAW call, so they move under stopped updates too;
 * rewind them as before (a new cursor value, uavtrack.RingSweep.rebind / seek).
 * The KL pass is two small launches between the gradient kernel and the finalize kernel; the ratios come from ratio_out
 * or, where the caller passes none, from [max_batch] floats of handle scratch.  That scratch is allocated when the stop is
 * first turned on and grown by uavtrack_learner_reserve (neither for use inside a capture); no update allocates or
 * synchronises.  While the stop is off every call enqueues exactly what it enqueued before.
 * The setting is host-side and read when an update is ENQUEUED, so a captured graph keeps the one it was captured with;
 * the latch is device state, so replays obey it.  Not part of checkpoints, and not carried by sharding's learner state.
 * Refusals on the host, enqueuing nothing: (set) a limit that is NaN or negative, a null kl_out or state with on != 0, a
 * UAVTRACK_LOSS_REFERENCE learner; (while on) an update that brings no log_mu (uavtrack_learner_update, _weighted,
 * _discounted, _stored with log_mu == NULL), every uavtrack_learner_grad* entry point and uavtrack_learner_apply: a
 * gradient row keeps its P + 8 words and has nowhere to carry a KL sum.
 * Cost on one MI355X: DESIGN.md section 9. */

/* on != 0: kl_out (DEVICE fp32 [1]) and state (DEVICE int32 [2]) are the caller's buffers, not copied and not owned, in
 * the style of uavtrack_learner_set_diagnostics: they must outlive the updates enqueued while they are installed, and the
 * caller zeroes state before the first update (or calls uavtrack_learner_kl_reset).  on == 0: off; the other arguments
 * are not read.  A refused call changes nothing. */
int uavtrack_learner_set_kl_stop(uavtrack_learner *learner, int32_t on, double limit, float *kl_out, int32_t *state);
/* on, limit, kl_out and state as they were last set ({0, +inf, NULL, NULL} at create and while off). */
int uavtrack_learner_get_kl_stop(uavtrack_learner *learner, int32_t *on, double *limit, float **kl_out, int32_t **state);
/* state <- {0, 0}: a one-thread kernel on `stream`, stream-ordered and capturable.  An error while the stop is off. */
int uavtrack_learner_kl_reset(uavtrack_learner *learner, void *stream);

/* Synchronises `stream`; fails if any update or apply since the previous check was refused on the device (bad action,
 * index, importance weight, discount, behaviour log-probability or ratio, a bad given advantage pair, a stored advantage
 * that is not finite, or a row of another layout).  refused (nullable) receives their number; the count restarts at 0. */
int uavtrack_learner_check(uavtrack_learner *learner, int64_t *refused, void *stream);

/* ---- the PMI trainer: PMINetwork.train_pmi + its Adam steps on the device ----
 * A handle of its own, independent of any environment.  It holds one reference PMINetwork (PMINet.py:20-62: three
 * branch Linear(5|4|3, H) + BatchNorm1d + ReLU blocks, concat, Linear(3H, H) + BatchNorm1d + ReLU, Linear(H, 1)) and
 * its torch.optim.Adam state (PMINet.py:39: lr, betas (0.9, 0.999), eps 1e-8).
 * State blob (uavtrack_pmi_trainer_num_params: n_state floats): the float entries of PMINetwork.state_dict() in its
 * order, H = hidden -- for each block (fc_comm/bn_comm, fc_obs/bn_obs, fc_boundary_state/bn_boundary_state, fc1/bn1):
 *   Linear.weight [H][in] (in = 5, 4, 3, 3H), Linear.bias [H], bn.weight [H], bn.bias [H], bn.running_mean [H],
 *   bn.running_var [H]
 * then fc2.weight [1][H], fc2.bias [1].  The four bn.num_batches_tracked entries travel as a separate int64 [4].
 * Adam blobs (n_train floats) hold the 18 trainable tensors in PMINetwork.parameters() order: per block Linear.weight,
 * Linear.bias, bn.weight, bn.bias, then fc2.weight, fc2.bias; step [18] is each tensor's Adam step count. */
typedef struct uavtrack_pmi_trainer_config {
    uint32_t struct_size;       /* = sizeof(uavtrack_pmi_trainer_config), ABI check */
    int32_t  device_id;         /* HIP device ordinal */
    int32_t  hidden;            /* H in [1, 256] (PMINet.py:21 hidden_dim; the scorer's limit) */
    int32_t  pad_;              /* 0 */
    int64_t  max_batch;         /* scratch for mini-batches up to this many rows; 0 = 4096 (uavtrack_pmi_trainer_reserve) */
    double   lr;                /* Adam learning rate (PMINet.py:39: 1e-3) */
} uavtrack_pmi_trainer_config;

typedef struct uavtrack_pmi_trainer uavtrack_pmi_trainer;   /* opaque handle */

/* Replaces PMINetwork.__init__ (PMINet.py:21-39).  Every state entry, moment and count starts at zero: upload the
 * initial state with uavtrack_pmi_trainer_set_params.  Allocates everything a train call needs. */
int uavtrack_pmi_trainer_create(const uavtrack_pmi_trainer_config *cfg, uavtrack_pmi_trainer **out);
int uavtrack_pmi_trainer_destroy(uavtrack_pmi_trainer *trainer);

/* Floats in the state blob (n_state) and in each Adam moment blob (n_train). */
int uavtrack_pmi_trainer_num_params(uavtrack_pmi_trainer *trainer, int64_t *n_state, int64_t *n_train);

/* Grows the scratch to mini-batches of max_batch rows (allocates; synchronises the device).  Never shrinks. */
int uavtrack_pmi_trainer_reserve(uavtrack_pmi_trainer *trainer, int64_t max_batch);

/* load_state_dict / state_dict: HOST blobs, state [n_state] in the order above and num_batches_tracked [4] (>= 0).
 * Synchronise `stream`.  A failing set leaves the previous state in place. */
int uavtrack_pmi_trainer_set_params(uavtrack_pmi_trainer *trainer, const float *state, const int64_t *num_batches_tracked,
                                    int64_t n_state, void *stream);
int uavtrack_pmi_trainer_get_params(uavtrack_pmi_trainer *trainer, float *state, int64_t *num_batches_tracked,
                                    int64_t n_state, void *stream);

/* optimizer.load_state_dict / state_dict: exp_avg, exp_avg_sq [n_train] and step [18] (int64, >= 0) as HOST blobs in
 * parameters() order.  Synchronise `stream`.  A failing set leaves the previous state in place. */
int uavtrack_pmi_trainer_set_optimizer_state(uavtrack_pmi_trainer *trainer, const float *exp_avg, const float *exp_avg_sq,
                                             const int64_t *step, int64_t n_train, void *stream);
int uavtrack_pmi_trainer_get_optimizer_state(uavtrack_pmi_trainer *trainer, float *exp_avg, float *exp_avg_sq,
                                             int64_t *step, int64_t n_train, void *stream);

/* Replaces PMINetwork.train_pmi (PMINet.py:74-100) after its index draw, stream-ordered: no synchronisation, no
 * allocation, capturable into a graph.  rows [n_rows][12] (DEVICE) is the observation history, timestep-major
 * (n_rows = T * n_uav); t_idx [b2] and u_idx [b2][2] (DEVICE, int64) are the drawn triples.  Mini-batch b of
 * batch_size rows takes input_1_2 row i = rows[t_idx[g] * n_uav + u_idx[g][0]], input_1_3 = rows[t_idx[g] * n_uav +
 * u_idx[g][1]], g = b * batch_size + i; each of the b2 / batch_size steps is zero_grad, two train-mode forwards,
 * CustomLoss, backward and one Adam step, the running statistics and step counts advancing on the device.
 * Outputs (DEVICE): avg_loss (fp32 scalar: the mean of |loss| over the steps); losses [b2 / batch_size] (nullable:
 * |loss| of each step); outputs [b2 / batch_size][2][batch_size] (nullable: output_1_2 and output_1_3 of each step).
 * Returns an error, enqueuing nothing, for a null required pointer, n_uav < 1, n_rows not a positive multiple of
 * n_uav, batch_size < 2, b2 < batch_size, or batch_size above the reserve.  A t_idx outside [0, T) or a u_idx outside
 * [0, n_uav) is found on the device: the call then changes nothing (state, moments, counts), its losses are NaN, and
 * the next uavtrack_pmi_trainer_check reports it. */
int uavtrack_pmi_trainer_train(uavtrack_pmi_trainer *trainer, const float *rows, int64_t n_rows, int64_t n_uav,
                               const int64_t *t_idx, const int64_t *u_idx, int64_t b2, int64_t batch_size,
                               float *avg_loss, float *losses, float *outputs, void *stream);

/* Synchronises `stream`; fails if any train call since the previous check was refused on the device (an index out
 * of range).  refused (nullable) receives their number; the count restarts at 0. */
int uavtrack_pmi_trainer_check(uavtrack_pmi_trainer *trainer, int64_t *refused, void *stream);

/* uavtrack_publish_pmi_weights from the trainer's own state into `env`'s scorer: stream-ordered, no synchronisation,
 * no allocation, capturable; the state is read when the launches execute, so a graph replayed after training
 * publishes the weights of that moment.  Refused, with nothing enqueued, if the two handles sit on different devices
 * or the trainer's hidden differs from the installed width. */
int uavtrack_pmi_trainer_publish(uavtrack_pmi_trainer *trainer, uavtrack_env *env, void *stream);

/* One observation history among several (K shard handles on one device, or the part of a timeline one rank holds).  A
 * *group* is n_uav consecutive rows: one "timestep" of train_pmi.  The *timeline* of sources[0..count) is the
 * concatenation of their groups in list order: group t lives in source k when base_k <= t < base_k + n_rows_k / n_uav,
 * base_k being the number of groups in the sources before k. */
typedef struct uavtrack_pmi_source {
    const float *rows;      /* DEVICE: [n_rows][12], timestep-major */
    int64_t n_rows;         /* a positive multiple of n_uav */
} uavtrack_pmi_source;

#define UAVTRACK_PMI_MAX_SOURCES 64

/* uavtrack_pmi_trainer_train on the timeline of sources[0..count), bit for bit (state, running statistics,
 * num_batches_tracked, both moments, step counts, avg_loss, losses, outputs); count == 1 is that call.  The rows are
 * never concatenated: one gather launch per scratch fill copies the 2 selected rows of each draw into the trainer's
 * scratch (as many draws as the reserve holds rows: one fill per call while b2 <= max_batch), and the step kernels run
 * on them.  Stream-ordered: no synchronisation, no allocation, capturable into a graph.  `sources` is a HOST array read
 * during the call and captured by value (the pointers and row counts, not the rows).
 * Returns an error, enqueuing nothing, for a count outside [1, UAVTRACK_PMI_MAX_SOURCES], a null rows, an n_rows that
 * is not a positive multiple of n_uav, and whatever uavtrack_pmi_trainer_train refuses.  A t_idx outside [0, total
 * groups) or a u_idx outside [0, n_uav) is found on the device, as there: the call changes nothing, its losses are NaN,
 * and the next uavtrack_pmi_trainer_check reports it. */
int uavtrack_pmi_trainer_train_many(uavtrack_pmi_trainer *trainer, const uavtrack_pmi_source *sources, int32_t count,
                                    int64_t n_uav, const int64_t *t_idx, const int64_t *u_idx, int64_t b2,
                                    int64_t batch_size, float *avg_loss, float *losses, float *outputs, void *stream);

/* The gather alone, for a participant that holds part of a timeline: sources[0..count) are the groups [group_base,
 * group_base + local groups) of a timeline of total_groups groups.  For every draw i whose t_idx[i] falls inside that
 * span, selected[i] ([b2][2][12], DEVICE) receives rows (t_idx[i], u_idx[i][0]) and (t_idx[i], u_idx[i][1]); the rows
 * of every other draw are left as they were.  Every draw is checked against total_groups and n_uav on the device: one
 * out of range makes the call write nothing, and the next uavtrack_pmi_trainer_check reports it.  Stream-ordered,
 * no synchronisation, no allocation, capturable; `sources` as above.  Returns an error, enqueuing nothing, for a bad
 * source list (as above), b2 outside [1, 2^31 - 1], group_base < 0 or a span that ends behind total_groups. */
int uavtrack_pmi_trainer_select(uavtrack_pmi_trainer *trainer, const uavtrack_pmi_source *sources, int32_t count,
                                int64_t group_base, int64_t total_groups, int64_t n_uav, const int64_t *t_idx,
                                const int64_t *u_idx, int64_t b2, float *selected, void *stream);

/* ---- the prioritised replay ring: PrioritizedReplayBuffer.add / sample on the device ----
 * The reference's PrioritizedReplayBuffer (train.py:73-139) as a ring of caller-owned DEVICE tensors: states and
 * next_states [capacity][12] fp32, actions [capacity] int32, rewards and priorities [capacity] fp32.  pos (next slot to
 * write) and count (valid slots) are host state: they follow from the number of transitions added alone, so the caller
 * advances them after each add (pos = (pos + n) % capacity, count = min(capacity, count + n)).  The handle owns only
 * scratch (tile sums, the draw counter, the status words, per-draw probabilities), all allocated at create.
 *
 * The draw stream.  Draw j (0 <= j < n) of the c-th sample call on a handle (c = 0, 1, ...; the counter lives on the
 * device and advances inside each call, so every replay of a captured graph draws afresh) takes
 *     (r0, r1, r2, r3) = Philox4x32-10(counter = (j, c mod 2^32, c >> 32, 0x52504C59 "RPLY"),
 *                                      key = (seed mod 2^32, seed >> 32))
 *     u = ((r0 << 21) | (r1 >> 11)) * 2^-53          (53 bits: u in [0, 1 - 2^-53])
 * Word 3 of the reset (0x55415631 "UAV1") and actor (0x4143544F "ACTO") streams differs, so no draw shares a counter with
 * them.  The slot is searchsorted(cdf, u * total, side='right') with w_i = p_i^alpha in fp32 (the reference's float32
 * `priorities ** alpha`), cdf its fp64 running sum over [0, count) and total = cdf[count - 1], as np.random.choice
 * (train.py:106).  Sums are exact for integer weights below 2^53; otherwise a draw within rounding of a CDF boundary
 * may fall on either side of it.  The rule there: a draw that rounding sends to a lane (32 slots) or a tile (2048
 * slots) holding no w > 0, or past the last w > 0 of the lane or tile it was sent to, takes the last slot with w > 0
 * at or before that lane or tile.  So a draw never lands on a slot >= count or one with w = 0.
 *
 * A uniform ring.  The reference's other buffer, ReplayBuffer (train.py:41-70), is the same ring without priorities:
 * ring->priorities == NULL.  The three adds then write the four stores alone, and the draw is
 * uavtrack_replay_sample_uniform (random.sample, train.py:56-58: without replacement); the prioritised draws refuse such
 * a ring.
 *
 * The uniform draw stream.  Draw j (0 <= j < n <= count) of call c -- the same device call counter as above: every
 * sample call of either kind reads it and advances it by one -- is pi_c(j), pi_c applied again while the value is
 * >= count.  pi_c is a bijection of [0, 2^b), b = the smallest even number >= 2 with 2^b >= count (so 2^b < 4 count from
 * count = 2 on), h = b / 2: a balanced Feistel network of 16 rounds on x = L * 2^h + R,
 *     (L, R) <- (R, L xor (fmix32((R + key_r) mod 2^32) mod 2^h))            for r = 0 .. 15, in this order
 *     fmix32(x): x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16   (mod 2^32; murmur3's finaliser)
 *     key_(4 i + w) = word w of Philox4x32-10(counter = (i, c mod 2^32, c >> 32, 0x554E4946 "UNIF"),
 *                                             key = (seed mod 2^32, seed >> 32))                 for i = 0 .. 3
 * and pi_c(x) = L * 2^h + R of the last round.  Word 3 differs from the three streams above.  The walk ends: it runs on
 * the cycle of pi_c through j, which holds j < count itself.  No two draws meet: two walks that met would, pi_c being a
 * bijection, have started from the same j.  So the n indices are distinct, and they are the first n entries, in order,
 * of a permutation of [0, count) that depends on (seed, c, count) alone: n = count gives all of it, a smaller n its
 * prefix.  Everything is integer arithmetic, so the indices are bitwise reproducible anywhere.  The expected number of
 * applications of pi_c per draw is 2^b / count < 4.
 *
 * The sweep stream (on-policy epochs: uavtrack_replay_sample_sweep).  A sweep goes through a window of the ring -- the
 * W = length slots first, first + 1, ... taken mod capacity -- in epochs of M = W / n (integer division) minibatches of
 * n slots, every slot at most once per epoch.  It is numbered by a cursor the caller owns (two DEVICE words), not by the
 * handle's call counter, which a sweep call neither reads nor advances: cursor[0] is the number q of the next call; a
 * one-thread kernel in front of the draw copies it to cursor[1] and advances it, so every replay of a captured graph
 * takes the next minibatch, and the draw reads q = cursor[1].  Call q is minibatch m = q mod M of epoch e = q / M, formed
 * on the device, and its entry j (0 <= j < n) is
 *     indices[j] = (first + sigma_e(m n + j)) mod capacity
 * sigma_e(x) being pi(x), pi applied again while the value is >= W, with pi the Feistel network of the uniform draw
 * stream above on b bits (b the smallest even number >= 2 with 2^b >= W): the same 16 rounds and fmix32, the round keys
 *     key_(4 i + w) = word w of Philox4x32-10(counter = (i, e mod 2^32, e >> 32, 0x53574550 "SWEP"),
 *                                             key = (seed mod 2^32, seed >> 32))                 for i = 0 .. 3
 * -- the epoch in the place of the call number, and a word 3 that differs from the four streams above.  As there, the
 * walks from the starts x < W end and never meet, so sigma_e is a permutation of [0, W): the M calls of an epoch return
 * M n distinct slots of the window, all of it when n divides W; otherwise the last W mod n entries of that epoch's
 * permutation are left out, other slots every epoch (a shuffled loader's drop_last).  Another epoch has other keys,
 * hence another order.  Everything is integer arithmetic, so the indices are bitwise reproducible anywhere, and depend
 * on (seed, q, first, W, n, capacity) alone: two cursors over the same window agree call for call. */
typedef struct uavtrack_replay_config {
    uint32_t struct_size;       /* = sizeof(uavtrack_replay_config), ABI check */
    int32_t  device_id;         /* HIP device ordinal */
    int64_t  max_capacity;      /* largest ring capacity this handle serves, >= 1 */
    int64_t  max_batch;         /* largest sample (draws per call), in [1, 2^31) */
    uint64_t seed;              /* Philox key of the draw stream */
} uavtrack_replay_config;

typedef struct uavtrack_replay uavtrack_replay;   /* opaque handle */

/* One ring: DEVICE pointers to the caller's stores and priorities, the capacity and the host-side pos and count. */
typedef struct uavtrack_replay_ring {
    float   *states;            /* [capacity][12] */
    int32_t *actions;           /* [capacity] */
    float   *rewards;           /* [capacity] */
    float   *next_states;       /* [capacity][12] */
    float   *priorities;        /* [capacity]; NULL: a uniform ring */
    int64_t  capacity;          /* in [1, max_capacity] */
    int64_t  pos;               /* in [0, capacity) */
    int64_t  count;             /* in [0, capacity] */
} uavtrack_replay_ring;

/* Replaces PrioritizedReplayBuffer.__init__'s state (train.py:74-81) beyond the caller's tensors.  Allocates all the
 * scratch the other calls use; synchronises the device. */
int uavtrack_replay_create(const uavtrack_replay_config *cfg, uavtrack_replay **out);
int uavtrack_replay_destroy(uavtrack_replay *replay);

/* ---- the adds (five, and the GAE add further down): what they share ----
 * An add writes n transitions into the caller's ring, in order f = 0 .. n - 1.  Only the last min(n, capacity) are
 * written, from slot (pos + max(0, n - capacity)) % capacity on, wrapping; on a ring with priorities each gets the
 * maximum of the whole priorities array as it stood before the call (1.0 when count == 0), taken on the device.
 * ring->priorities may be NULL (a uniform ring): the call then reads and writes no priority and writes the stores
 * exactly as otherwise.  The ring struct is the caller's and is not advanced: pos and count move on the caller's side.
 * Every array is DEVICE memory.  Stream-ordered, no synchronisation, no allocation, capturable.
 * Errors.  Each add returns an error, enqueuing nothing, for the first of these that applies: a null handle; a ring
 * that is null, lacks a store, has its states or next_states off a 16-byte boundary, or is outside the limits above; a
 * null pointer among those the form requires; exactly one of done and start_obs where both are optional; a source row
 * array ([..][12]) off a 16-byte boundary; n_step, then lambda, then gamma out of range where the form has them; a size
 * below 1; sizes whose product overflows.  Each entry point below states what it adds to this.
 *
 * uavtrack_replay_add: PrioritizedReplayBuffer.add (train.py:87-96) for n transitions given flat: states / next_states
 * [n][12], actions [n] int32, rewards [n], all required. */
int uavtrack_replay_add(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, const float *states,
                        const int32_t *actions, const float *rewards, const float *next_states, void *stream);

/* The same add straight from one rollout (uavtrack_run_actor's outputs, train.py:176-180): obs_in [agents][12] is what
 * the policy saw first, obs [steps][agents][12], actions and reward [steps][agents] (agents = n_envs * n_uav).
 * Transition f = t * agents + i (t < steps) is (state = t ? obs[t - 1][i] : obs_in[i], actions[t][i], reward[t][i],
 * next_state = obs[t][i]), the [t][b][i] order of uavtrack.transitions_from_rollout; n = steps * agents.  Each obs row
 * is read once.  All four arrays are required. */
int uavtrack_replay_add_rollout(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t steps, int64_t agents,
                                const float *obs_in, const float *obs, const int32_t *actions, const float *reward,
                                void *stream);

/* uavtrack_replay_add_rollout for a rollout that crossed episode ends (uavtrack_run_actor_autoreset): envs * n_uav
 * agents per step, done [steps][envs] (uint8) and start_obs [steps][envs][n_uav][12] as that launch wrote them.  The
 * state of transition (t, b, i) is obs_in[b][i] at t == 0, start_obs[t - 1][b][i] where done[t - 1][b] != 0 (the
 * episode of step t - 1 ended there: its last observation is not the state step t acted on), else obs[t - 1][b][i].
 * done and start_obs are required here.  Everything else is uavtrack_replay_add_rollout's; each obs row is still read
 * once, a start_obs row only where done fired.  With done all zero the ring ends byte-identical to
 * uavtrack_replay_add_rollout's (start_obs is then never read). */
int uavtrack_replay_add_rollout_episodes(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t steps,
                                         int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                         const int32_t *actions, const float *reward, const uint8_t *done,
                                         const float *start_obs, void *stream);

/* ---- multi-step targets: n-step returns from one rollout ----
 * uavtrack_replay_add_rollout_episodes with each transition's reward folded over the next n steps of its agent.
 * A rollout has steps = T and envs * n_uav agents per step; transition (t, b, i) is flattened as
 * f = t * agents + b * n_uav + i, the order of uavtrack_replay_add_rollout.  n = n_step in
 * [1, UAVTRACK_REPLAY_MAX_NSTEP]; g = (float)gamma, gamma finite and in [0, 1].
 *   Horizon.  m(t, b) is the smallest m >= 1 for which one of these holds: m == n, t + m == T, or
 *     done[t + m - 1][b] != 0.  A window never crosses an episode end, and it is cut at the rollout's last step, so every
 *     step still yields exactly one transition.  Without done only the first two conditions apply.  The horizon depends
 *     on (t, b) alone.
 *   Return.  fp32 Horner from the far end, every multiply and add rounded on its own (no fused multiply-add):
 *     R = reward[t + m - 1][b][i]; for k = m - 2 ... 0: R = reward[t + k][b][i] + g * R.
 *   Discount.  d = g; then d = d * g exactly m - 1 times, in fp32.
 *   Stored transition.  state: exactly what uavtrack_replay_add_rollout_episodes stores for (t, b, i) -- obs_in at t == 0,
 *     start_obs[t - 1] behind a fired done, obs[t - 1] otherwise; action = actions[t][b][i]; reward = R;
 *     next_state = obs[t + m - 1][b][i] (at an episode end that episode's last observation, which is what the one-step
 *     form bootstraps from); discount = d, written to discounts [capacity], a caller-owned DEVICE fp32 array passed
 *     beside the ring (the ring struct keeps its size).  Slot, window, wrap and priority are the shared ones; the
 *     windows of the written transitions still look ahead into rows that are themselves not written.
 * With n == 1: m == 1 everywhere, R is the reward's bits and d is g's bits; the four stores and the priorities end
 * byte-identical to uavtrack_replay_add_rollout_episodes, and with done == NULL to uavtrack_replay_add_rollout.
 * done and start_obs are either both given or both NULL; discounts and the four rollout arrays are required.  One thread
 * handles one transition: it reads at most n rewards and n - 1 done bytes, one next-state row and its state row. */
#define UAVTRACK_REPLAY_MAX_NSTEP 64
int uavtrack_replay_add_rollout_nstep(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                      int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                      const int32_t *actions, const float *reward, const uint8_t *done,
                                      const float *start_obs, int32_t n_step, double gamma, void *stream);

/* ---- TD(lambda) targets: lambda-returns from one rollout ----
 * uavtrack_replay_add_rollout_episodes with each transition stored as a (reward, discount) pair whose one-step target
 * is the lambda-return.  T = steps, agents = envs * n_uav, f = t * agents + b * n_uav + i as above.
 * values [T][envs][n_uav] is a caller-given DEVICE fp32 array meant to hold V(obs[t][b][i]), the value of the state step
 * t ends in (at an episode end that episode's last observation, which is what the one-step form bootstraps from;
 * uavtrack_learner_values over obs gives it).  g = (float)gamma and l = (float)lambda, both finite and in [0, 1];
 * gl = g * l and c = g * (1.0f - l).  Every operation is rounded to fp32 on its own (no fused multiply-add).
 * Per agent chain (b, i), walking t = T - 1 ... 0 and carrying G:
 *     cut(t) = (t == T - 1) || (done != NULL && done[t][b] != 0) || (gl == 0)
 *     cut:     R_t = reward[t][b][i]               d_t = g
 *     else:    R_t = reward[t][b][i] + gl * G      d_t = c
 *     G = R_t + d_t * values[t][b][i]
 * Stored transition (t, b, i): state, action and priority exactly as uavtrack_replay_add_rollout_episodes stores them
 * (without done and start_obs: as uavtrack_replay_add_rollout); next_state = obs[t][b][i]; reward = R_t; discount = d_t,
 * written to discounts [capacity] as the n-step add writes its own.  Slots, the window for T * agents > capacity and the
 * wrap are those of the other adds; the chain still walks rows that are themselves not written.
 * The learner's target of such a slot (uavtrack_learner_update_discounted) is
 *     R_t + d_t V_now(s'_t) = r_t + g l G_{t+1} + g (1 - l) V_now(s_{t+1}),
 * the lambda-return with its tail G_{t+1} evaluated by the critic as it stood at add time and its first bootstrap term
 * by the critic at update time.  Slots keep the tail they were added with (stale tails are accepted, as in caches of
 * lambda-returns under replay).  A window never crosses an episode end and is cut at the rollout's last step, where the
 * transition is the one-step one.  d_t is in [0, 1].  With lambda == 0 or gamma == 0 every step is a cut and all five
 * stores and the priorities end byte-identical to uavtrack_replay_add_rollout_nstep at n_step == 1 (a reward of -0.0
 * included: a cut copies the reward, it does not add zero to it).  With lambda == 1, d_t == 0 inside a segment:
 * Monte-Carlo up to the cut, the bootstrap at the cut.  Non-finite values propagate into the stored rewards as non-finite
 * rewards do; the add does not inspect them.
 * The one-step write runs first; a scan kernel follows it, one thread per agent chain, the loads of eight steps issued
 * ahead of the carried G.  The horizon is unbounded.  Required and optional arrays are those of
 * uavtrack_replay_add_rollout_nstep, with values required as well. */
int uavtrack_replay_add_rollout_lambda(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                       int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                       const int32_t *actions, const float *reward, const uint8_t *done,
                                       const float *start_obs, const float *values, double lambda, double gamma,
                                       void *stream);

/* ---- fixed GAE(lambda) advantages and value targets per slot: what PPO epochs train on ----
 * uavtrack_replay_add_rollout_lambda with three more arrays and one more store.  Beyond values (as above):
 *   values_in    [envs][n_uav]     DEVICE fp32, V(obs_in);
 *   values_start [T][envs][n_uav]  DEVICE fp32, V(start_obs[t]); NULL together with done and start_obs, and read only
 *                                  where done[t][b] fired;
 *   advantages   [capacity]        DEVICE fp32, caller-owned, passed beside the ring like discounts (the ring struct keeps
 *                                  its size): the seventh per-slot store.
 * The fold is the lambda add's, operation for operation: the same g, l, gl, c, the same cut(t), R_t and d_t, and
 *     G = R_t + d_t * values[t][b][i]            (every operation rounded to fp32 on its own)
 * Stored transition (t, b, i): state, action, next_state and priority exactly what the lambda add stores;
 *   reward    = G_t, the bits the fold forms for G at step t: the lambda-return with EVERY term evaluated at add time;
 *   discount  = +0.0f, so the learner's target r + d V(s') of the slot is the fixed value target G_t (PPO's
 *               returns = advantages + values; d == 0 is "do not bootstrap", which the learner already handles);
 *   advantage = fl(G_t - Vs_t), Vs_t the value of the state the step began in: values_in[b][i] at t == 0,
 *               values_start[t - 1][b][i] where done[t - 1][b] fired, values[t - 1][b][i] otherwise.
 * Since sum_k (g l)^k delta_{t+k} = G^lambda_t - V(s_t) with delta_t = r_t + g V(s_{t+1}) - V(s_t), the advantage is
 * GAE(lambda).  It bootstraps at the rollout's last step and at a fired done: done is the horizon, a truncation, as the
 * lambda add treats it.  On the same inputs the states, actions, next_states and priorities end byte-identical to the
 * lambda add's and reward == fl(R_t + fl(d_t * values[t])) of its (R_t, d_t).
 * Slots, the window for T * agents > capacity and the wrap are those of the other adds.  The one-step write runs first; a
 * scan kernel of its own follows, one thread per agent chain, the loads of eight steps issued ahead of the carried G
 * (the lambda add's kernels are not touched).  Non-finite values propagate; the add does not inspect them (the learner
 * refuses a drawn advantage that is not finite, uavtrack_learner_update_stored).
 * Required: discounts, advantages, the four rollout arrays, values, values_in.  done, start_obs and values_start are all
 * given or all NULL.  lambda, gamma, sizes and alignment as uavtrack_replay_add_rollout_lambda. */
int uavtrack_replay_add_rollout_gae(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                    float *advantages, int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in,
                                    const float *obs, const int32_t *actions, const float *reward, const uint8_t *done,
                                    const float *start_obs, const float *values, const float *values_in,
                                    const float *values_start, double lambda, double gamma, void *stream);

/* PrioritizedReplayBuffer.sample's draw (train.py:98-112) without the gather: n slots with replacement from
 * P(i) = p_i^alpha / sum_j p_j^alpha over [0, count) (the draw stream above) into indices [n] (DEVICE int64), and,
 * if weights (DEVICE fp32 [n]) is not NULL, the importance weights (count * P(i))^-beta / max over the batch, computed
 * in fp64.  Only ring->priorities and ring->count are used.  Stream-ordered, no synchronisation, no allocation,
 * capturable; indices and weights are bitwise reproducible for the same seed and call number.  Returns an error,
 * enqueuing nothing, for a null pointer, n < 1 or n > max_batch, count < 1 or count > capacity or capacity >
 * max_capacity, alpha not finite and > 0, or beta not finite and >= 0.  A priority in [0, count) that is NaN,
 * infinite or negative, or an all-zero [0, count), is found on the device: the call then writes slot 0 to every index
 * and NaN weights, and the next uavtrack_replay_check reports it. */
int uavtrack_replay_sample(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, double alpha,
                           double beta, int64_t *indices, float *weights, void *stream);

/* uavtrack_replay_sample with beta read off a linear schedule on the device, so that a captured draw anneals when its
 * graph is replayed.  Call number c is the device call counter uavtrack_replay_sample uses and advances (both calls
 * share it), read before it advances; call c uses
 *   beta_c = beta0 + (beta1 - beta0) * min(1, c / anneal_calls)
 * formed in fp64 on the device, each operation rounded on its own (no fused multiply-add), so the same expression in
 * host doubles gives the same beta_c and uavtrack_replay_sample at beta_c the same bits.  anneal_calls >= 1; beta0 and
 * beta1 finite and >= 0.  Everything else -- the draw stream, the refusals, the errors, capturability -- is
 * uavtrack_replay_sample's contract. */
int uavtrack_replay_sample_annealed(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, double alpha,
                                    double beta0, double beta1, int64_t anneal_calls, int64_t *indices, float *weights,
                                    void *stream);

/* ReplayBuffer.sample's draw (train.py:56-58, random.sample) without the gather: n DISTINCT slots of [0, count), in
 * random order, into indices [n] (DEVICE int64) -- the uniform draw stream above.  Only ring->count (and the limits
 * ring->capacity and ring->pos are checked against) is used; ring->priorities may be NULL.  The work is O(n) whatever
 * the ring holds.  Stream-ordered, no synchronisation, no allocation, capturable; the call advances the handle's call
 * counter as the prioritised draws do, so a replayed graph draws afresh.  Returns an error, enqueuing nothing and leaving
 * the counter alone, for a null handle, ring or indices, n < 1 or n > max_batch, count < 1, n > count, count > capacity
 * or capacity > max_capacity.  It reads no ring data, so nothing is refused on the device. */
int uavtrack_replay_sample_uniform(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, int64_t *indices,
                                   void *stream);

/* The next minibatch of a sweep over a ring window (the sweep stream above): n distinct slots of the window of `length`
 * slots from `first` on (wrapping at ring->capacity) into indices [n] (DEVICE int64), numbered by cursor (DEVICE, 2
 * uint64 words, the caller's: word 0 the number of the next call, to be set -- 0 to begin, q to go to call q -- by the
 * caller on the same stream; word 1 scratch).  length / n consecutive calls return every slot of the window exactly once
 * when n divides length, and length / n * n distinct ones otherwise.  Only ring->capacity and ring->count (and
 * ring->pos, checked against the limits) are used; it reads no ring data, so nothing is refused on the device, and
 * ring->priorities may be NULL or not.  The work is O(n).  Stream-ordered, no synchronisation, no allocation,
 * capturable; the handle's call counter is neither read nor advanced, so the other draws' streams are what they are
 * without any sweep.  Returns an error, enqueuing nothing and leaving the cursor alone, for a null handle, ring, cursor
 * or indices, n < 1 or n > max_batch, count < 1, count > capacity or capacity > max_capacity, length < 1, first outside
 * [0, capacity), n > length, or a window that leaves the valid slots: length > count or, while count < capacity,
 * first + length > count (a full ring's window may wrap). */
int uavtrack_replay_sample_sweep(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t first, int64_t length,
                                 int64_t n, uint64_t *cursor, int64_t *indices, void *stream);

/* Synchronises `stream`; fails if any sample call since the previous check was refused on the device (bad or all-zero
 * priorities).  refused (nullable) receives their number; the count restarts at 0. */
int uavtrack_replay_check(uavtrack_replay *replay, int64_t *refused, void *stream);

/* ---- per-episode results: ReturnValueOfTrain on the device, across automatic resets ----
 * The reference reports six results per episode (train.py:181-196, appended by train, evaluate and run through
 * ReturnValueOfTrain, train.py:12-38).  This handle, independent of any environment, folds the outputs a stepping
 * launch has already written -- reward [T][B][N], terms [T][3][B][N], covered [T][B], done [T][B] -- into per-environment
 * open-episode accumulators that live on the device and carry over from call to call, and appends one record per
 * finished episode to a device log.  It reads the FINAL reward array, so it is the same for MAAC, MAAC-G and MAAC-R.
 *
 * Arithmetic.  Every sum is fp64 in one fixed order: the N values of a step are added in ascending UAV index i,
 * starting from +0.0 (Python's sum(reward_list[...]), train.py:181-184), and the step sums are added to the episode's
 * accumulator in ascending t (train.py:181 `+=`).  The covered sum (int64) and maximum (int32) are integers.  The
 * division happens once, when the record is written: sum / (double)(steps * N), (double)covered_sum / (double)steps.
 * An episode is limited to 2^31 - 1 steps.
 *
 * Order of the log.  The records of one add appear in ascending (t, b) of their closing step: the order of a scan over
 * the done matrix, not of arrival.  The records of one close appear in ascending b.  Two identical call sequences give
 * byte-identical logs.
 *
 * Overflow.  Once the log holds log_capacity records, further records are counted, not written; their episodes'
 * accumulators restart all the same.  The read call returns that count in `dropped`. */
typedef struct uavtrack_episode_stats_config {
    uint32_t struct_size;       /* = sizeof(uavtrack_episode_stats_config), ABI check */
    int32_t  device_id;         /* HIP device ordinal */
    int64_t  n_envs;            /* B >= 1 */
    int32_t  n_uav;             /* N in [1, 2048] */
    int32_t  pad_;              /* 0 */
    int64_t  env_offset;        /* global id of env 0 (shards): record.env = env_offset + b */
    int64_t  max_steps;         /* largest T of one add; sizes the step-sum scratch (max_steps * n_envs < 2^31) */
    int64_t  log_capacity;      /* records the device log holds, >= 1 */
} uavtrack_episode_stats_config;

typedef struct uavtrack_episode_record {   /* 64 bytes, no padding */
    double  ret, tracking, boundary, duplicate;   /* each episode sum / (steps * N)                 (train.py:187-190) */
    double  average_covered, max_covered;         /* np.mean / np.max of covered over the episode's steps (train.py:191-192) */
    int64_t env;                                  /* env_offset + b */
    int32_t steps;                                /* steps in this episode */
    int32_t ordinal;                              /* episodes this environment had closed before this one */
} uavtrack_episode_record;

typedef struct uavtrack_episode_stats uavtrack_episode_stats;   /* opaque handle */

/* Allocates the accumulators (all zero: every environment starts with an open episode of no steps, ordinal 0), the
 * step-sum scratch and the log; synchronises the device. */
int uavtrack_episode_stats_create(const uavtrack_episode_stats_config *cfg, uavtrack_episode_stats **out);
int uavtrack_episode_stats_destroy(uavtrack_episode_stats *stats);

/* Folds the T steps of one launch (DEVICE pointers, the layouts above; done nullable) into the open episodes.  Step t of
 * environment b first joins the open episode; if done[t][b] != 0 the episode closes with that step included: its record
 * goes to the log, the accumulators restart and the environment's ordinal advances.  With done == NULL nothing closes.
 * Stream-ordered: no synchronisation, no allocation, capturable into a graph; the arrays are read when the launches
 * execute on `stream`.  Under MAAC-R it belongs behind the stepping call, whose last stage writes the final rewards.
 * Returns an error, enqueuing nothing, for a null handle, reward, terms or covered, T < 1 or T > max_steps.  A
 * negative covered count, or one above 2^31 - 1, is not checked. */
int uavtrack_episode_stats_add(uavtrack_episode_stats *stats, int64_t T, const float *reward, const float *terms,
                               const int32_t *covered, const uint8_t *done, void *stream);

/* Ends every open episode that holds at least one step, as a done flag behind its last step would have: for
 * fixed-length rollouts whose caller resets by hand and never sees done (train.py:160 with num_steps).  Stream-ordered
 * like the add. */
int uavtrack_episode_stats_close(uavtrack_episode_stats *stats, void *stream);

/* Synchronises `stream`.  *count = the records the log holds; the first min(*count, capacity) of them are copied, in
 * log order, to records_host (a HOST array of `capacity` records; may be NULL when capacity is 0).  *dropped = the
 * records that found the log full since the last clear. */
int uavtrack_episode_stats_read(uavtrack_episode_stats *stats, uavtrack_episode_record *records_host, int64_t capacity,
                                int64_t *count, int64_t *dropped, void *stream);

/* Empties the log and zeroes `dropped`, stream-ordered.  The open episodes and the ordinals stay as they are. */
int uavtrack_episode_stats_clear(uavtrack_episode_stats *stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* UAVTRACK_H */

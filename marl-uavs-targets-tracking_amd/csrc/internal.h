// internal.h -- shared between the C-ABI translation unit and the kernel files.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "uavtrack.h"

namespace uavtrack {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kTwoPi = 6.28318530717958647692f;
constexpr int kMaxWorkgroup = 512;   // __launch_bounds__ of the rollout kernel
constexpr size_t kLdsSoft = 64 * 1024;    // dynamic LDS a launch gets without asking
constexpr size_t kLdsMax = 160 * 1024;    // LDS of a gfx950 CU: what one workgroup may take (hipFuncAttributeMaxDynamicSharedMemorySize)
constexpr int kSymBits = 20;         // fixed-point bits of the shared duplicate term (step_kernel.hip, sym_dup): e * 2^20 < 2^22

// Kernel arguments of one rollout launch (T >= 1 steps).  All pointers are device
// pointers.  Derived constants are computed once on the host in fp64, then cast.
// The state arrays live in ONE device slab at offsets that follow from (B, N, M, dim), so the kernel
// carries a single base pointer (2 SGPRs instead of 20 through the whole step loop) and derives the
// rest with scalar adds -- no dependent pointer load at the start of a launch.  Slab order (4-byte
// units): ux uy uh ua [uz] (B*N each), tx ty th [tz] (B*M each), step_count (B), episode (B), climb_c climb_s (8 each).
struct StateBlock {
    // state, SoA over (env, uav) and (env, target); updated in place
    float *ux, *uy, *uz, *uh;
    int32_t *ua;
    float *tx, *ty, *tz, *th;
    int32_t *step_count;
    int32_t *episode;           // episode number of each environment's last reset (keys the next automatic one)
    float *climb_c, *climb_s;   // cos/sin of the climb angles (UAVTRACK_MAX_CLIMB each)
};

__host__ __device__ inline StateBlock state_view(float *slab, int B, int N, int M, bool z3)
{
    const size_t BN = (size_t)B * N, BM = (size_t)B * M;
    StateBlock v;
    float *f = slab;
    v.ux = f; f += BN;
    v.uy = f; f += BN;
    v.uh = f; f += BN;
    v.ua = reinterpret_cast<int32_t *>(f); f += BN;
    v.uz = z3 ? f : nullptr; if (z3) f += BN;
    v.tx = f; f += BM;
    v.ty = f; f += BM;
    v.th = f; f += BM;
    v.tz = z3 ? f : nullptr; if (z3) f += BM;
    v.step_count = reinterpret_cast<int32_t *>(f); f += B;
    v.episode = reinterpret_cast<int32_t *>(f); f += B;
    v.climb_c = f; f += UAVTRACK_MAX_CLIMB;
    v.climb_s = f;
    return v;
}
inline size_t state_slab_floats(int B, int N, int M, bool z3)
{
    return ((size_t)B * N) * (z3 ? 5 : 4) + ((size_t)B * M) * (z3 ? 4 : 3) + 2 * (size_t)B + 2 * UAVTRACK_MAX_CLIMB;
}

struct StepParams {
    float *slab;             // state slab, see state_view()
    // per-step I/O, leading [T] axis
    const int32_t *actions;
    float *obs, *reward, *terms;
    float2 *tpos;            // optional target trace [T][B][M] (x, y) after each step (uavtrack_set_target_trace)
    float *raw;              // optional raw rewards [T][B][N]: uav.raw_reward of environment.py:219 (uavtrack_set_raw_reward_output)
    float *state_copy;       // optional second copy of the state slab as it stands behind the launch (uavtrack_step_host: the host block)
    uint32_t *nbrec;         // MAAC-R: neighbour record per agent-step, read by the deferred softmax mix (nbrec_words())
    int32_t *covered;
    uint8_t *done;
    float *ep_sums;
    uint2 *pairs;            // MAAC-R: neighbour pair list {flat [t][b][i] index of i, that of j}, i < j (0xFFFFFFFF: slot-pool dummy)
    unsigned *pair_count;
    unsigned long long *pair_total;   // accounting: neighbour pairs emitted so far (uavtrack_pmi_pairs_scored)
    // geometry
    int32_t B, N, M, E, T, na, na_total, horizon;
    int32_t ep_accumulate;   // 1: ep_sums += (uavtrack_step_accumulate), 0: ep_sums = sums of this launch
    // automatic episode turnover (uavtrack_step_many_autoreset): an environment whose done flag fires is reset in place
    int32_t auto_reset;      // 0, kAutoResetOn, or kAutoResetContinued for the later chunks of a chunked launch (MAAC-R)
    uint32_t reset_k0, reset_k1;     // reset seed (Philox key), as uavtrack_reset
    double x_max_d, y_max_d, z_max_d;
    // fused greedy rollout (uavtrack_run_greedy): actions come from the in-kernel baseline policy
    int32_t *actions_out;    // [T][B][N], nullable
    int64_t env_offset;
    uint32_t greedy_k0, greedy_k1;   // policy seed (greedy and actor rollouts)
    // fused actor rollout (uavtrack_run_actor): actions come from the in-kernel policy network (actor.h)
    const float *obs_in;     // [B][N][12] observation seen at the first step
    const float *actor_w;    // packed weight blob
    int32_t actor_hblocks, actor_mode;   // 32-unit tiles of the hidden layer
    // constants
    float x_max, y_max, z_max;
    float dtv_u, dtv_t;          // dt * v_max of UAVs / targets
    float turn_unit;             // dt * h_max / (na - 1)        (uav.py:81,96)
    float inv_dc, inv_dp, dp, dp2, dc2, two_dp2;
    float le_neg_scale, le_dp2, le_dc2, le_two_dp2;   // pk_le_mask: -S and nextafter(K) * S per threshold
    float lt_dp2;                                     // strict form: K * S  (d2 < K)
    float vratio;                // target.v_max / uav.v_max      (uav.py:116)
    float inv_na_total;
    float inv_na;                // 1 / na: the climb index of a 3-D action is floor((a + 0.5) / na)
    float act_bias, inv_act_bias;   // step_kernel.hip act_bias_shape(): K, a power of two above n_uav * na * nc, and 1 / K
    float exp_k0, exp_k1;        // exp((2dp-d)/(2dp)) = exp2(k0 - k1*d)   (uav.py:226)
    float sym_k0;                // step_kernel.hip sym_dup: k0 + b, b = kSymBits the fixed-point bits of the shared duplicate term
    float tt_ceil, inv_tt_ceil;  // 2*m_targets                   (environment.py:208)
    float dup_k, sym_dup_k;      // the duplicate term's clip and normalisation folded (environment.py:210,217): dup = clamp(k * sum g, -1, 0)
                                 // with k = -0.5 / (e/2 * n_uav) for a float sum of g, times 2^-kSymBits for sym_dup's fixed-point sum
    float alpha, beta, gamma, coop;
    // automatic reset: optional [T][B][N][12] observation of the fresh state, written at the steps whose done flag fired
    // (uavtrack_set_start_obs_output).  Last member: the kernel-argument offsets of everything above stay where they were.
    float *start_obs;
};
constexpr int32_t kAutoResetOn = 1, kAutoResetContinued = 2;

// MAAC-R neighbour record of one agent-step, 32-bit words: [0 .. W) neighbour bit mask (d <= dp on post-move poses,
// uav.py:278; bit j = UAV j, self excluded), [W] index of the first pair this UAV emitted (its neighbours j > i, in
// ascending j, occupy consecutive slots of the pair list / score array; isolated pairs are not emitted).  W = 1 up to 32
// UAVs (one 8-byte record), 2 up to 64, else ceil(N / 32).  The UAV's raw reward travels in the REWARD output slot of the
// step (step_kernel.hip, pmi_reward_slot): raw while it has neighbours, the final reward when it has none.
__host__ __device__ inline int nbrec_mask_words(int N) { return N <= 32 ? 1 : (N <= 64 ? 2 : (N + 31) / 32); }
__host__ __device__ inline int nbrec_words(int N) { return nbrec_mask_words(N) + 1; }

struct PmiWeights {
    float *blob = nullptr;   // device, folded layout of uavtrack_set_pmi_weights; behind it the bf16 planes of fc1
    const void *x6 = nullptr; // -> into blob: fc1 as three bf16 planes in MFMA operand order (pack_pmi_x6), or null
    const void *l1 = nullptr; // -> into blob: the branch layers as f16 planes in MFMA A-operand order (pack_pmi_l1), with t3
    const void *t3 = nullptr; // -> into blob: fc1 block-scaled as two f16 planes (f16(T w), remainder) for pmi_score_t3_kernel,
                              //    or null when the network's weights / activation bounds do not fit f16's range
    const float *scal = nullptr;   // -> into blob: the scalar block (pmi_pack.h): block scales, range-watch limits, f16 verdict
    float *fold = nullptr;   // device scratch of a device publish (pmi_pack_kernel.hip): the folded network, n_floats floats
    // a device publish (uavtrack_publish_pmi_weights) has written the allocation since the last uavtrack_set_pmi_weights:
    // l1 / t3 are then set whatever the verdict, which only the device knows (the scalar block), and AUTO / F16X3 launch
    // the t3 kernel with its gated stand-by
    bool dev_published = false;
    int32_t hidden = 0;      // padded to the scorer's granule
    int32_t hidden_raw = 0;  // as given to uavtrack_set_pmi_weights
    size_t n_floats = 0;
};

struct Geometry {
    int wgs = 0;          // threads per workgroup
    int envs_per_wg = 0;  // E
    int groups = 0;       // workgroups
    size_t lds_bytes = 0;
    int specialised = 0;
    int lone = 0;         // single-wave groups on a grid of at most two waves per SIMD: the LONE kernel variant
};

// The template arguments of one rollout_kernel instantiation, in the kernel's own order: N_, M_ (0, 0: the generic
// kernel), MODE as instantiated, Z3, POLICY, ALLOUT, EXTRAS, LONE.  Written where the function pointer is taken
// (step_kernel.hip, pick_reward), nowhere else; all -1 until a launch has happened (uavtrack_variant_info: all zeros is a
// real kernel).
struct VariantInfo { int64_t v[8] = {-1, -1, -1, -1, -1, -1, -1, -1}; };

}  // namespace uavtrack

struct uavtrack_env {
    uavtrack_config cfg;
    uavtrack::StepParams base;   // constants filled at create
    float *slab = nullptr;       // the one device allocation behind `state`
    uavtrack::StateBlock state;  // pointers into the slab (host-side view)
    uavtrack::Geometry geo;
    // MAAC-R launches of fewer than kPmiShortLaunch steps, or without a single-wavefront variant (select_rollout): the 4-wave
    // geometry (one pair-list reservation per workgroup-step on a quarter of the workgroups; the single-wavefront variant's
    // block reservations pay off over many steps, and a launch that starts with an empty pool waits for its first one)
    uavtrack::Geometry geo_short;
    uavtrack::Geometry last_launch;   // geometry of the most recent rollout launch (uavtrack_launch_info)
    uavtrack::VariantInfo last_variant;   // ... and the kernel instantiation it ran (uavtrack_variant_info)
    uavtrack::PmiWeights pmi;
    int32_t n_cus = 0;           // compute units of the device (grid of the persistent scorer)
    int32_t pmi_scheme = 0;      // uavtrack_set_pmi_scheme: UAVTRACK_PMI_AUTO or a pinned scorer
    unsigned *pmi_flags = nullptr;   // device [3]: the f16 scorer's range flag; chunks re-scored by the wide-range kernel because an
                                     // input left f16's range at run time; chunks it scored because published weights do not fit f16
    float *actor_w = nullptr;    // device blob of uavtrack_set_actor_weights (actor.h layout)
    double *actor_scales = nullptr;   // device [2]: T1, T2 between the two launches of a device publish (actor_pack_kernel.hip)
    int32_t actor_hidden = 0;
    // MAAC-R scratch for `pmi_steps_cap` steps of deferred scoring (rewards never feed back into the
    // dynamics, so a chunk of steps is simulated first and all its pairs are scored in one launch):
    // pair list + counter, one score per pair, neighbour records [steps][B][N], and
    // observation / term buffers for callers that pass NULL
    int32_t pmi_steps_cap = 0;
    uint2 *pairs = nullptr;
    unsigned *pair_count = nullptr;
    unsigned long long *pair_total = nullptr;
    float *scores = nullptr, *obs_tmp = nullptr;   // scores: one per emitted pair
    uint32_t *nbrec = nullptr;
    float2 *tpos = nullptr;           // caller's target-trace buffer (not owned), capacity in steps
    int32_t tpos_steps = 0;
    float *raw_out = nullptr;         // caller's raw-reward buffer (not owned), capacity in steps (uavtrack_set_raw_reward_output)
    int32_t raw_steps = 0;
    float *start_obs_out = nullptr;   // caller's fresh-state observation buffer (not owned), capacity in steps (uavtrack_set_start_obs_output)
    int32_t start_obs_steps = 0;
    float *state_copy_out = nullptr;  // (during uavtrack_step_host) where the launch leaves a second copy of the state slab
    // uavtrack_step_host: one pinned, device-mapped host block (actions in, every output and a copy of the state out)
    void *host_blk = nullptr;         // host address (hipHostMalloc)
    void *host_blk_dev = nullptr;     // the same block as the device sees it (hipHostGetDevicePointer)
    size_t host_blk_bytes = 0;
    float *rsum = nullptr;            // [steps][B] per-step mean of the final reward (mix kernel -> episode return)
    // uavtrack_set_profiling: a HIP event pair on the launch stream around every kernel launch of the stepping entry points,
    // by kernel class (UAVTRACK_PROF_*); read and cleared by uavtrack_get_profile
    struct ProfRec { int cls; hipEvent_t a, b; };
    bool profiling = false;
    std::vector<ProfRec> prof;
    // uavtrack_pmi_inference scratch (grow-only): [2 n][12] scorer inputs and the n pair records
    float *inf_obs = nullptr;
    uint2 *inf_pairs = nullptr;
    size_t inf_cap = 0;
};

namespace uavtrack {

// step_kernel.hip
Geometry plan_geometry(const uavtrack_config &cfg, int n_simd, bool allow_small_grid = true);
enum { kPolicyGiven = 0, kPolicyGreedy = 1, kPolicyActor = 2 };   // where a rollout's actions come from
// one rollout launch of p.T steps: the kernel variant and the geometry (env->geo or env->geo_short) are chosen by
// select_rollout; the choice is kept in env->last_launch and env->last_variant
hipError_t launch_rollout(uavtrack_env *env, const StepParams &p, hipStream_t stream, int policy = kPolicyGiven);

// pmi_kernel.hip
constexpr int kPmiShortLaunch = 16;
constexpr int kPmiMaxHidden = 256;                  // widest PMINetwork hidden layer the scorer is instantiated for
inline int pmi_padded_hidden(int hidden) { return (hidden + 31) / 32 * 32; }   // the scorer's column-block granule
void pack_pmi_blob(const float *abi_blob, float *device_order, int hidden);
constexpr int kPmiX6MaxHidden = 128;                // widest layer whose three bf16 planes stay register-resident (4 waves, one per SIMD)
constexpr int kPmiX6MinHidden = 64;                 // (narrower layers have fewer k-steps than the producer has pairs to hide)
inline size_t pmi_x6_floats(int hp) { return hp >= kPmiX6MinHidden && hp <= kPmiX6MaxHidden ? (size_t)3 * hp * hp * 3 / 2 : 0; }   // 3 planes x 2 B
void pack_pmi_x6(const float *abi_blob, uint16_t *planes, int hidden);
inline size_t pmi_t3_floats(int hp) { return hp >= kPmiX6MinHidden && hp <= kPmiX6MaxHidden ? (size_t)3 * hp * hp : 0; }   // 2 planes x 2 B
void pack_pmi_t3(const float *abi_blob, uint16_t *planes, int hidden, float T);
inline size_t pmi_l1_floats(int hp) { return pmi_t3_floats(hp) ? (size_t)(hp / 32) * 3 * 3 * 64 * 8 / 2 : 0; }   // [w][branch][3 planes][lane][8] x 2 B
void pack_pmi_l1(const float *abi_blob, uint16_t *planes, int hidden, float S1);
// (pairs / scores / n_uav default to the handle's MAAC-R scratch and swarm size; uavtrack_pmi_inference passes its own)
hipError_t launch_pmi_score(const uavtrack_env *env, const float *obs, hipStream_t stream, const uint2 *pairs = nullptr,
                            float *scores = nullptr, int n_uav = 0);
int pmi_effective_scheme(const uavtrack_env *env);              // enum uavtrack_pmi_scheme, never AUTO
bool pmi_scheme_available(const uavtrack_env *env, int scheme);
bool pmi_scheme_fits(int hidden_padded, bool f16_range_ok, int scheme);   // the same test for weights that are not loaded yet
hipError_t launch_pmi_counters_reset(const uavtrack_env *env, hipStream_t stream);
hipError_t launch_pmi_inference_prep(const float *x, float *obs2, uint2 *pairs, unsigned n, hipStream_t stream);
hipError_t launch_pmi_finalize(const uavtrack_env *env, int steps, float *reward, float *rsum, hipStream_t stream);
hipError_t launch_ep_reward(const uavtrack_env *env, int steps, const float *rsum, float *ep_sums, bool add, hipStream_t stream);

// policy_kernel.hip
hipError_t launch_greedy(const uavtrack_env *env, uint64_t seed, int32_t *actions, hipStream_t stream);
hipError_t launch_actor(const uavtrack_env *env, const float *obs, uint64_t seed, int mode, int32_t *actions,
                        float *probs, hipStream_t stream);

// actor_pack_kernel.hip -- pack_actor_blob (actor.h) restated on the device: fp32 DEVICE weights in torch layouts -> the
// actor blob, two stream-ordered launches.  `scales` holds the block scales T1, T2 (fp64) between the two.
struct ActorPackArgs {
    const float *w1, *b1, *w2, *b2;    // [H][12], [H], [A][H], [A]
    int H, A, at;                      // hidden units, actions, action tiles of the blob
    double xb[UAVTRACK_OBS_DIM];       // nominal bounds of |obs_k| (actor_obs_bounds)
    float *blob;                       // actor_blob_floats(H, at) floats
    double *scales;                    // [2]
};
hipError_t launch_actor_pack(const ActorPackArgs &a, hipStream_t stream);

// reset_kernel.hip
hipError_t launch_reset(const uavtrack_env *env, uint64_t seed, uint32_t episode, float *obs,
                        hipStream_t stream);

// What both device trainers (uavtrack_learner_*, uavtrack_pmi_trainer_*) keep the same way: the torch.optim.Adam state
// of their trainable tensors and the words through which a call is refused on the device.  api.hip owns its buffers
// (adam_bufs), loads and reads it (optimizer_state) and takes the refusals (take_refusals).
struct AdamState {
    int tensors = 0, P = 0;         // trainable tensors, their floats
    float *m = nullptr, *v = nullptr;   // [P] exp_avg, exp_avg_sq
    int64_t *steps = nullptr;       // [tensors] Adam step per trainable tensor
    int *status = nullptr;          // [1] this call's input errors
    int *errors = nullptr;          // [1] calls refused since the last *_check
};

// torch.optim.Adam (defaults: betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad), the single-tensor and
// foreach forms' arithmetic: m.lerp_(g, 1 - b1); v = v * b2 + (1 - b2) g^2; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// with bc = 1 - b^step in double precision on the host side of torch (here: on the device, from the device step count).
// One element: w, m, v are updated in place from the gradient g at Adam step `step` (already advanced for this step).
__device__ __forceinline__ void adam_element(float &w, float &m, float &v, float g, int64_t step, float lr)
{
    const double s = (double)step;
    const double bc1 = 1.0 - pow(0.9, s), bc2 = 1.0 - pow(0.999, s);
    const float step_size = (float)((double)lr / bc1);
    const float bc2_sqrt = (float)sqrt(bc2);
    float mi = m;
    mi = mi + 0.1f * (g - mi);                              // lerp with weight 1 - 0.9 < 0.5
    const float vi = v * 0.999f + 0.001f * g * g;
    const float denom = sqrtf(vi) / bc2_sqrt + 1e-8f;
    w = w - step_size * (mi / denom);
    m = mi;
    v = vi;
}

// learner_kernel.hip -- the device learner (uavtrack_learner_*).  Both networks' parameters live in one fp32 array in
// torch order: actor fc1.weight [H][12], fc1.bias [H], fc2.weight [A][H], fc2.bias [A], then critic fc1.weight [H][12],
// fc1.bias [H], fc2.weight [1][H], fc2.bias [1]; the Adam moments use the same order.
constexpr int kLearnerTensors = 8;
constexpr int kLearnerMaxHidden = 256;
constexpr int kLearnerMaxActions = 48;
constexpr int kLearnerMaxGroups = 256;        // workgroups of the gradient kernel (= gradient partial rows)
constexpr int kLearnerRowTail = 8;            // words behind the P gradient sums of a gradient row: 4 loss sums, n (2), status, P
struct LearnerLayout {
    int H, A, P;
    int a_w1, a_b1, a_w2, a_b2, c_w1, c_b1, c_w2, c_b2;
    static LearnerLayout make(int H, int A)
    {
        LearnerLayout L;
        L.H = H; L.A = A;
        L.a_w1 = 0; L.a_b1 = 12 * H; L.a_w2 = 13 * H; L.a_b2 = 13 * H + A * H;
        L.c_w1 = L.a_b2 + A; L.c_b1 = L.c_w1 + 12 * H; L.c_w2 = L.c_b1 + H; L.c_b2 = L.c_w2 + H;
        L.P = L.c_b2 + 1;
        return L;
    }
    __host__ __device__ int offset(int t) const
    {
        const int o[kLearnerTensors] = {a_w1, a_b1, a_w2, a_b2, c_w1, c_b1, c_w2, c_b2};
        return o[t];
    }
    __host__ __device__ int tensor_of(int p) const
    {
        int t = 0;
        while (t + 1 < kLearnerTensors && p >= offset(t + 1)) ++t;
        return t;
    }
};
// the device state of one learner handle
struct LearnerDevice {
    LearnerLayout L;
    float gamma, actor_lr, critic_lr;
    int per_sample;
    float *params;                  // [P]
    AdamState opt;                  // kLearnerTensors tensors over [P]; opt.status: the last update's / apply's verdict
    int *gstatus;                   // [1] input errors of the last uavtrack_learner_grad (they travel in its row)
    float *partials;                // [kLearnerMaxGroups][P + 4]
    float *scal;                    // [2] gradient scales of the current update
    float *td;                      // [max_n] td_delta when the caller passes none
    uint8_t *last;                  // [max_n] last-occurrence marks of the priority write
    int64_t max_n;
    // regularisation (uavtrack_learner_set_regularisation / _set_diagnostics): host-side settings, read at enqueue
    float entropy_coef;             // c >= 0; != 0 only with per_sample
    double max_norm[2];             // actor, critic: > 0, +inf = off
    float *entropy;                 // caller's [entropy_rows] buffer (not owned) or null
    int64_t entropy_rows;
    float *grad_norm;               // caller's [2] buffer (not owned) or null
    float *gsum;                    // [P] the scaled gradient of a clipped update
    double *sq;                     // [learner_clip_groups][2] its workgroups' sums of squares: actor, critic
    float *coef;                    // [2] the clip coefficients
};
struct LearnerLaunch {
    int64_t n, capacity;
    const float *states, *rewards, *next_states;
    const int32_t *actions;
    const int64_t *idx;
    const float *weights;           // nullable [n]: importance weights in batch order
    const float *discounts;         // nullable [capacity]: per-slot discounts (null: the handle's gamma for every row)
    float *actor_loss, *critic_loss, *td_delta, *priorities;
};
int learner_rows_per_tile(int hidden);
size_t learner_lds_bytes(const LearnerLayout &L, int rows);
int learner_groups(const LearnerLayout &L, int64_t n);
int learner_clip_groups(const LearnerLayout &L);   // workgroups of the clip's gradient pass: ceil(P / 256)
hipError_t learner_prepare_kernels(const LearnerLayout &L);
hipError_t launch_learner_update(const LearnerDevice &d, const LearnerLaunch &q, hipStream_t stream);
// the split update: gradient row [P + kLearnerRowTail] <- one batch; rows [count][P + kLearnerRowTail] -> both Adam steps;
// the priority write gated on the last apply's verdict
hipError_t launch_learner_grad(const LearnerDevice &d, const LearnerLaunch &q, float *row, hipStream_t stream);
hipError_t launch_learner_apply(const LearnerDevice &d, const float *rows, int count, float *actor_loss,
                                float *critic_loss, hipStream_t stream);
hipError_t launch_learner_priorities(const LearnerDevice &d, const int64_t *idx, int64_t n, int64_t capacity,
                                     const float *td, float *prio, hipStream_t stream);
// uavtrack_learner_values: values[i] = V(rows[i]) with the critic as it stands when the launch executes, the chain of
// the gradient kernel's V(s) to the bit; no scratch, any n >= 1
hipError_t launch_learner_values(const LearnerDevice &d, int64_t n, const float *rows, float *values, hipStream_t stream);

// pmi_train_kernel.hip -- the device PMI trainer (uavtrack_pmi_trainer_*).  `state` holds the float entries of the
// reference PMINetwork's state_dict in its order (26 tensors: per Linear+BatchNorm1d block weight, bias, bn weight, bn
// bias, running_mean, running_var; then fc2.weight, fc2.bias); the gradients and Adam moments hold the 18 trainable
// tensors in PMINetwork.parameters() order (per block weight, bias, bn weight, bn bias; then fc2).
constexpr int kPmiTrainTensors = 18;
constexpr int kPmiStateTensors = 26;
constexpr int kPmiBlocks = 4;                 // fc_comm, fc_obs, fc_boundary_state, fc1 (each with a BatchNorm1d)
constexpr int64_t kPmiTrainMaxBatch = (int64_t)1 << 20;
struct PmiTrainLayout {
    int H, S, P;
    int soff[kPmiStateTensors + 1];           // state tensor offsets (soff[26] = S)
    int poff[kPmiTrainTensors + 1];           // trainable tensor offsets (poff[18] = P)
    __host__ __device__ static int state_of(int t) { return t < 16 ? (t / 4) * 6 + t % 4 : t + 8; }
    static PmiTrainLayout make(int H)
    {
        PmiTrainLayout L;
        L.H = H;
        const int in[kPmiBlocks] = {5, 4, 3, 3 * H};
        int ssz[kPmiStateTensors], k = 0;
        for (int b = 0; b < kPmiBlocks; ++b) {
            ssz[k++] = H * in[b];
            for (int q = 0; q < 5; ++q) ssz[k++] = H;
        }
        ssz[k++] = H;
        ssz[k++] = 1;
        L.soff[0] = 0;
        for (int t = 0; t < kPmiStateTensors; ++t) L.soff[t + 1] = L.soff[t] + ssz[t];
        L.poff[0] = 0;
        for (int t = 0; t < kPmiTrainTensors; ++t) L.poff[t + 1] = L.poff[t] + ssz[state_of(t)];
        L.S = L.soff[kPmiStateTensors];
        L.P = L.poff[kPmiTrainTensors];
        return L;
    }
};
// the device state of one trainer handle
struct PmiTrainDevice {
    PmiTrainLayout L;
    float lr;
    float *state;                   // [S] state_dict floats
    int64_t *nbt;                   // [4] num_batches_tracked per BatchNorm1d
    float *grad;                    // [P]
    AdamState opt;                  // kPmiTrainTensors tensors over [P]
    // per-step scratch, feature-major ([side][feature][row]) for batches up to max_b rows
    float *xh0, *a0, *da0;          // [2][3H][max_b] branch BN: normalised input, post-ReLU output, dL/d(output)
    float *xh1, *a1, *dz1;          // [2][H][max_b]  bn1: normalised input, post-ReLU output; dL/d(fc1 output)
    float *inv0, *inv1;             // [2][3H], [2][H] 1 / sqrt(var + eps) of the current step
    float *go;                      // [2][max_b] dL/d(output_1_2), dL/d(output_1_3)
    float *acc;                     // [1] sum of |loss| over the call
    // uavtrack_pmi_trainer_train_many: the selected rows of up to max_b draws and the identity triples that address them
    float *sel;                     // [max_b][2][12]
    int64_t *sel_t, *sel_u;         // [max_b] = i, [max_b][2] = (0, 1)
    int64_t max_b;
};
struct PmiTrainLaunch {
    const float *rows;
    int64_t n_rows, n_uav, b2, batch;
    const int64_t *t_idx, *u_idx;
    float *avg_loss, *losses, *outputs;
};
hipError_t launch_pmi_train(const PmiTrainDevice &d, const PmiTrainLaunch &q, hipStream_t stream);
// A source list as the select kernel takes it, by value: source k holds the timeline's groups [base[k], base[k + 1])
constexpr int kPmiMaxSources = 64;            // UAVTRACK_PMI_MAX_SOURCES
struct PmiSourceTable {
    const float *rows[kPmiMaxSources];
    int64_t base[kPmiMaxSources + 1];         // base[0]: the span's first group in the timeline
    int count;
};
// uavtrack_pmi_trainer_train_many: q.rows is unused, q.n_rows = total groups * n_uav
hipError_t launch_pmi_train_many(const PmiTrainDevice &d, const PmiSourceTable &src, const PmiTrainLaunch &q,
                                 hipStream_t stream);
// uavtrack_pmi_trainer_select: the draws of the table's span into selected [b2][2][12]
hipError_t launch_pmi_select(const PmiTrainDevice &d, const PmiSourceTable &src, int64_t total_groups, int64_t n_uav,
                             const int64_t *t_idx, const int64_t *u_idx, int64_t b2, float *selected, hipStream_t stream);

// replay_kernel.hip -- the prioritised replay ring (uavtrack_replay_*).  The ring's stores and priorities belong to the
// caller; the handle owns the scratch below.  Sampling works on tiles of kReplayTile slots: per-tile fp64 sums, one
// inclusive scan of them, then one wavefront per draw (binary search over the tile prefix, rescan of one tile).
constexpr int kReplayTile = 2048;
constexpr int kReplayMaxParts = 1024;         // workgroups of the priority-maximum reduction
constexpr uint32_t kReplayDomain = 0x52504C59u;   // "RPLY": Philox counter word 3 of the draw stream
constexpr uint32_t kUniformDomain = 0x554E4946u;  // "UNIF": Philox counter word 3 of the uniform draw's round keys
constexpr int kUniformRounds = 16;            // Feistel rounds of the uniform draw's bijection (four Philox blocks of keys)
struct ReplayDevice {
    int64_t max_capacity, max_batch;
    uint32_t k0, k1;                // Philox key: the ring's seed
    double *prefix;                 // [ceil(max_capacity / kReplayTile)] tile sums, then their inclusive prefix
    int64_t *tile_last;             // [same] last slot of a tile with a non-zero weight, -1 if none
    uint64_t *counter;              // [2] call counter (advanced on the device), this call's value
    unsigned long long *pmin;       // [1] smallest sampled P(i) of this call (fp64 bits)
    double *pdraw;                  // [max_batch] P(i) of each draw
    float *parts;                   // [kReplayMaxParts] per-workgroup priority maxima; [kReplayMaxParts] = the maximum
    int *status;                    // [1] this call's refusal bits
    int *errors;                    // [1] draws refused since the last check
};
struct ReplayRingView {
    float *states, *rewards, *next_states, *priorities;
    int32_t *actions;
    int64_t capacity, pos, count;
};
// beta of call c (the device counter before it advances): beta0 when anneal_calls == 0, else
// beta0 + (beta1 - beta0) * min(1, c / anneal_calls), formed in fp64 on the device
hipError_t launch_replay_sample(const ReplayDevice &d, const float *priorities, int64_t count, int64_t k, float alpha,
                                double beta0, double beta1, int64_t anneal_calls, int64_t *indices, float *weights,
                                hipStream_t stream);
// k distinct slots of [0, count), count <= 2^bits: the first k images of the call's keyed bijection, walked below count.
// Shares the call counter with launch_replay_sample.
hipError_t launch_replay_sample_uniform(const ReplayDevice &d, int64_t count, int64_t k, int64_t *indices,
                                        hipStream_t stream);
// One ring add of steps x envs x n_uav transitions, of which the last min(n, capacity) land in the ring from ring.pos on;
// ring.priorities == nullptr (a uniform ring): the stores alone.
//   Flat     states / next [n][12], actions / rewards [n], with steps = n and envs = n_uav = 1;
//   Rollout  obs_in [agents][12], next = obs [steps][agents][12], actions / rewards [steps][agents]; with done [steps][envs]
//            and start_obs (of obs's shape) the rollout crossed episode ends, without them envs * n_uav is just `agents`;
//   Nstep    Rollout's source folded into n_step-step returns with gamma; discounts [capacity] receives gamma^m per slot;
//   Lambda   Rollout's write, then the backward scan over each agent's chain that overwrites the written slots' rewards
//            with R_t and leaves d_t in discounts; values [steps][agents].
enum class ReplayForm { Flat, Rollout, Nstep, Lambda };
struct ReplayAdd {
    ReplayForm form;
    ReplayRingView ring;
    int64_t steps, envs, n_uav;
    const float *obs_in, *states, *next, *rewards;
    const int32_t *actions;
    const uint8_t *done;            // both given or both nullptr
    const float *start_obs;
    float *discounts;
    const float *values;
    int n_step;                     // n-step form: in [1, UAVTRACK_REPLAY_MAX_NSTEP]
    float lambda, gamma;
};
hipError_t launch_replay_add(const ReplayDevice &d, const ReplayAdd &q, hipStream_t stream);

// episode_kernel.hip -- per-episode results (uavtrack_episode_stats_*).  The open episodes are struct-of-arrays over the
// environments; a closing step's log slot comes from a scan over the done matrix in groups of kEpisodeGroup environments
// (one wavefront each).
constexpr int kEpisodeGroup = 64;
constexpr int kEpisodeMaxUav = 2048;          // a tile of one environment's four planes must fit the staging LDS
struct EpisodeDevice {
    int64_t B, env_offset, max_steps, log_capacity;
    int N;
    double *step_sums;              // [max_steps][4][B] per-step sums over the UAVs: reward, tracking, boundary, duplicate
    double *acc;                    // [4][B] the open episodes' sums
    int64_t *cov_sum;               // [B]
    int32_t *cov_max, *steps, *ordinal;   // [B] each
    uint32_t *slots;                // [max_steps * groups] closing steps per (t, group), then their exclusive prefix
    int64_t *head;                  // [3] records in the log, records dropped, the log's fill when the current call began
    uavtrack_episode_record *log;   // [log_capacity]
};
inline int64_t episode_groups(int64_t B) { return (B + kEpisodeGroup - 1) / kEpisodeGroup; }
hipError_t launch_episode_add(const EpisodeDevice &d, int64_t T, const float *reward, const float *terms,
                              const int32_t *covered, const uint8_t *done, hipStream_t stream);
hipError_t launch_episode_close(const EpisodeDevice &d, hipStream_t stream);

}  // namespace uavtrack

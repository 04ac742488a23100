// learner.h -- the device learner (uavtrack_learner_*): what learner_kernel.hip and api_learner.hip share.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "adam.h"

namespace uavtrack {

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
    // the target critic (uavtrack_learner_set_target): host-side settings, read at enqueue
    float *target;                  // [14 H + 1] the critic's block in torch order at offsets 0, 12 H, 13 H, 14 H; null
                                    // until a target is first enabled, then kept for the handle's life
    int target_mode;                // UAVTRACK_TARGET_OFF / _POLYAK / _PERIODIC
    float target_tau, target_omt;   // Polyak: (float)tau and 1.0f - (float)tau
    int64_t target_period;          // periodic: >= 1; 0 while Polyak
    // the normalised advantage (uavtrack_learner_set_advantage): host-side settings, read at enqueue
    int adv_mode;                   // kAdvantageRaw / _Batch / _Given (= enum uavtrack_advantage_mode); != raw only with per_sample
    double adv_eps;                 // batch: inv_std = 1 / (std + eps)
    const float *adv_given;         // given: the caller's [2] {mean, inv_std} (not owned), read when the launch executes
    float *adv_stats;               // [3] {mean, inv_std, std} of the last batch-mode update or grad ...
    float *adv_user;                // ... unless the caller installed a [3] buffer of its own (not owned), else null
    float *stats() const { return adv_user ? adv_user : adv_stats; }
    float *adv_td;                  // [max_n] the TD pass's delta; null until a mode other than raw is first set
    double *adv_part;               // [2][learner_adv_chunks(max_n)] the chunks' sums of delta, then of squared deviations
    float *adv_unit;                // [2] {0.0f, 1.0f}: the pair a stored advantage in raw mode is "standardised" by
    // KL early stopping (uavtrack_learner_set_kl_stop): host-side settings, read at enqueue; the latch is device state
    int kl_on;
    float kl_limit;                 // (float)limit: the update is stopped where kl > kl_limit in fp32 (+inf: never)
    float *kl_out;                  // caller's [1] (not owned): the last evaluated batch's KL estimate
    int32_t *kl_state;              // caller's [2] (not owned): {stopped (the latch), skipped}
    float *kl_ratio;                // [max_n] the ratios when the caller passes no ratio_out; null until the stop is first on
    double *kl_part;                // [learner_adv_chunks(max_n)] the chunks' sums of k_i
};
constexpr int kLearnerStopped = 256;   // status bit 8: the update was stopped by the KL latch (not an error)
enum { kAdvantageRaw = 0, kAdvantageBatch = 1, kAdvantageGiven = 2 };
// One batch of uavtrack_learner_update / _grad in any of their forms.  The ten entry points fill it as they were
// called (the first nine fields in this order, by aggregate initialisation); what a form does not take stays zero.
struct LearnerLaunch {
    int64_t n, capacity;
    const float *states, *rewards, *next_states;
    const int32_t *actions;
    const int64_t *idx;
    const float *weights;           // nullable [n]: importance weights in batch order
    const float *discounts;         // nullable [capacity]: per-slot discounts (null: the handle's gamma for every row)
    bool clipped;                   // a _clipped entry point: log_mu is required, clip_eps is tested
    double clip_eps;                // as given; an accepted launch carries it folded into clip_lo / clip_hi
    const float *log_mu;            // nullable [capacity]: per-slot behaviour log-probabilities; non-null: the clipped surrogate
    float clip_lo, clip_hi;         // its bounds 1 - eps and 1 + eps in fp32 (read only with log_mu)
    float *ratio;                   // nullable [n]: its ratios in batch order (read only with log_mu)
    bool stored;                    // a _stored entry point: advantages is required, log_mu nullable, per-sample only
    const float *advantages;        // nullable [capacity]: per-slot advantages of the actor; non-null: the stored kernels
    float *actor_loss, *critic_loss, *td_delta, *priorities;
};
int learner_rows_per_tile(int hidden);
// extra_floats_per_row: a variant's lds_extra (learner_variants.h), behind the rest
size_t learner_lds_bytes(const LearnerLayout &L, int rows, int extra_floats_per_row = 0);
int learner_groups(const LearnerLayout &L, int64_t n);
int learner_clip_groups(const LearnerLayout &L);   // workgroups of the clip's gradient pass: ceil(P / 256)
int64_t learner_adv_chunks(int64_t n);             // 256-row chunks of the advantage statistics: ceil(n / 256)
inline int learner_critic_words(const LearnerLayout &L) { return 14 * L.H + 1; }   // the critic's block, c_w1 .. P
hipError_t learner_prepare_kernels(const LearnerLayout &L);
hipError_t launch_learner_update(const LearnerDevice &d, const LearnerLaunch &q, hipStream_t stream);
// the split update: gradient row [P + kLearnerRowTail] <- one batch; rows [count][P + kLearnerRowTail] -> both Adam steps;
// the priority write gated on the last apply's verdict
hipError_t launch_learner_grad(const LearnerDevice &d, const LearnerLaunch &q, float *row, hipStream_t stream);
hipError_t launch_learner_apply(const LearnerDevice &d, const float *rows, int count, float *actor_loss,
                                float *critic_loss, hipStream_t stream);
// uavtrack_learner_kl_reset: the latch and the skipped count back to 0, stream-ordered
hipError_t launch_learner_kl_reset(const LearnerDevice &d, hipStream_t stream);
hipError_t launch_learner_priorities(const LearnerDevice &d, const int64_t *idx, int64_t n, int64_t capacity,
                                     const float *td, float *prio, hipStream_t stream);
// uavtrack_learner_values: values[i] = V(rows[i]) with the critic as it stands when the launch executes, the chain of
// the gradient kernel's V(s) to the bit; no scratch, any n >= 1.  target: with the target critic's block (d.target)
hipError_t launch_learner_values(const LearnerDevice &d, bool target, int64_t n, const float *rows, float *values,
                                 hipStream_t stream);

}  // namespace uavtrack

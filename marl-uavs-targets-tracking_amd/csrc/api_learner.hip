// api_learner.hip -- the C ABI of the device learner (include/uavtrack.h, uavtrack_learner_*).
// The ten batch entry points (update, grad and their _weighted, _discounted, _clipped and _stored forms) each fill a
// LearnerLaunch as they were called and share one acceptor and one runner: accept_learner_batch, run_learner_batch.

#include "api_env.h"
#include "api_handle.h"
#include "learner.h"
#include "learner_policy.h"

#include <cmath>

using namespace uavtrack;

struct uavtrack_learner {
    uavtrack_learner_config cfg;
    LearnerDevice d;
    double reg[3] = {0.0, INFINITY, INFINITY};   // uavtrack_learner_get_regularisation: the values as they were set
    double target_tau = 0.0;                     // uavtrack_learner_get_target: tau as it was set (0 unless Polyak)
    double kl_limit = INFINITY;                  // uavtrack_learner_get_kl_stop: the limit as it was set
};

namespace uavtrack {

// the TD pass of a batch-normalised advantage: not part of a handle until a mode other than raw is first set
static Bufs advantage_bufs(LearnerDevice &d, int64_t max_n)
{
    return {buf(d.adv_td, max_n), buf(d.adv_part, 2 * (size_t)learner_adv_chunks(max_n))};
}

// the KL pass of the early stop: not part of a handle until the stop is first turned on
static Bufs kl_bufs(LearnerDevice &d, int64_t max_n)
{
    return {buf(d.kl_ratio, max_n), buf(d.kl_part, (size_t)learner_adv_chunks(max_n))};
}

static Bufs scratch_bufs(LearnerDevice &d, int64_t max_n)
{
    Bufs set = {buf(d.td, max_n), buf(d.last, max_n)};
    if (d.adv_td) set = set + advantage_bufs(d, max_n);
    return d.kl_ratio ? set + kl_bufs(d, max_n) : set;
}

static Bufs device_bufs(LearnerDevice &d)
{
    const size_t P = (size_t)d.L.P;
    return adam_bufs(d.opt) + Bufs{buf(d.params, P, true), buf(d.gstatus, 1, true), buf(d.partials, kLearnerMaxGroups * (P + 4)), buf(d.scal, 2),
                                   buf(d.gsum, P), buf(d.sq, 2 * (size_t)learner_clip_groups(d.L)), buf(d.coef, 2),
                                   buf(d.adv_stats, 3, true), buf(d.adv_unit, 2)} +
           scratch_bufs(d, d.max_n);
}

// the target critic's block: not part of device_bufs(), it is allocated when a target is first enabled
static Bufs target_bufs(LearnerDevice &d) { return {buf(d.target, (size_t)learner_critic_words(d.L))}; }

static int *refusal_word(const LearnerDevice &d) { return d.opt.errors; }

}  // namespace uavtrack

namespace {

constexpr int64_t kLearnerDefaultBatch = 65536;
constexpr int64_t kLearnerMaxBatch = ((int64_t)1 << 31) - 1;   // row numbers are int32 in the priority write

// The batch tests of uavtrack_learner_update / _grad / _write_priorities, after their null tests: n, the reserved
// scratch, the store's capacity, and n against it when no indices choose the rows (`dir`: "from" or "into" the store).
int accept_batch(const char *fn, const uavtrack_learner *l, int64_t n, int64_t capacity, const int64_t *indices,
                 const char *dir)
{
    if (n < 1) return fail("%s: n = %lld < 1", fn, (long long)n);
    if (n > l->d.max_n)
        return fail("%s: n = %lld rows, scratch is reserved for %lld (uavtrack_learner_reserve)", fn, (long long)n,
                    (long long)l->d.max_n);
    if (capacity < 1) return fail("%s: capacity = %lld < 1", fn, (long long)capacity);
    if (!indices && n > capacity)
        return fail("%s: n = %lld rows without indices %s a store of %lld", fn, (long long)n, dir, (long long)capacity);
    return 0;
}

// uavtrack_learner_update / _grad while an entropy buffer is installed: the batch must fit into it
int accept_entropy_rows(const char *fn, const uavtrack_learner *l, int64_t n)
{
    if (l->d.entropy && n > l->d.entropy_rows)
        return fail("%s: n = %lld rows, the installed entropy buffer holds %lld (uavtrack_learner_set_diagnostics)", fn,
                    (long long)n, (long long)l->d.entropy_rows);
    return 0;
}

// uavtrack_learner_update / _grad under a batch-normalised advantage: a standard deviation needs two rows
int accept_advantage_rows(const char *fn, const uavtrack_learner *l, int64_t n)
{
    if (l->d.adv_mode == UAVTRACK_ADVANTAGE_BATCH && n < 2)
        return fail("%s: n = %lld row under UAVTRACK_ADVANTAGE_BATCH: the standard deviation of a batch needs n >= 2 "
                    "(uavtrack_learner_set_advantage)", fn, (long long)n);
    return 0;
}

// what a per-row factor of the actor's gradient (`what`, a per-row `factor`) meets on a reference-loss learner
int refuse_on_reference(const char *fn, const char *what, const char *factor)
{
    return fail("%s: %s on a UAVTRACK_LOSS_REFERENCE learner: that form scales the actor's gradient sums once by "
                "-mean(delta) / N, a factor a per-row %s cannot share; use UAVTRACK_LOSS_PER_SAMPLE", fn, what, factor);
}

enum class Batch { Update, Grad };

// Every host-side refusal of the ten batch entry points (uavtrack_learner_update, _grad and their _weighted,
// _discounted, _clipped and _stored forms), in one order: the tests all forms share, a _stored call's own, then the
// clip's wherever a log_mu is required (_clipped) or given (_stored; without one clip_eps is not read).  Nothing has
// been enqueued when one of them fires.
int accept_learner_batch(const char *fn, const uavtrack_learner *l, const LearnerLaunch &q, Batch kind, const float *row)
{
    if (!l) return fail("%s: null handle", fn);
    if (!q.states || !q.actions || !q.rewards || !q.next_states)
        return fail("%s: states, actions, rewards and next_states must not be null", fn);
    if (kind == Batch::Update && (!q.actor_loss || !q.critic_loss))
        return fail("%s: actor_loss and critic_loss must not be null", fn);
    if (kind == Batch::Grad && (!q.td_delta || !row)) return fail("%s: td_delta and row must not be null", fn);
    if (accept_batch(fn, l, q.n, q.capacity, q.idx, "from") || accept_entropy_rows(fn, l, q.n) ||
        accept_advantage_rows(fn, l, q.n))
        return 1;
    if (q.stored) {
        if (!q.advantages) return fail("%s: advantages must not be null", fn);
        if (!l->d.per_sample) return refuse_on_reference(fn, "stored advantages", "advantage");
    }
    if (l->d.kl_on && kind == Batch::Grad)
        return fail("%s: KL early stopping is on (uavtrack_learner_set_kl_stop): a gradient row has nowhere to carry a KL "
                    "sum, so the split update is refused; use a closed clipped update, or turn the stop off", fn);
    if (l->d.kl_on && !q.log_mu)
        return fail("%s: KL early stopping is on (uavtrack_learner_set_kl_stop): the estimate is formed from the ratios "
                    "against log_mu, and this form brings none; use uavtrack_learner_update_clipped, or _update_stored "
                    "with a log_mu", fn);
    if (q.clipped || q.log_mu) {
        if (!q.log_mu) return fail("%s: log_mu must not be null", fn);
        if (!(q.clip_eps >= 0)) return fail("%s: clip_eps = %g must be >= 0 (+inf: never clips)", fn, q.clip_eps);
        if (!l->d.per_sample) return refuse_on_reference(fn, "the clipped surrogate", "gate");
    }
    return 0;
}

// The ten entry points behind their own names: accepted, the clip's bounds folded to fp32, then the closed update
// (row null) or the gradient half into `row`.
int run_learner_batch(const char *fn, uavtrack_learner *learner, LearnerLaunch q, Batch kind, float *row, void *stream)
{
    if (accept_learner_batch(fn, learner, q, kind, row)) return 1;
    ON_DEVICE(learner->cfg.device_id);
    if (q.log_mu) {
        const float eps32 = (float)q.clip_eps;
        q.clip_lo = 1.0f - eps32; q.clip_hi = 1.0f + eps32;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(kind == Batch::Update ? launch_learner_update(learner->d, q, st) : launch_learner_grad(learner->d, q, row, st));
    return 0;
}

// uavtrack_learner_values (target false) and _values_target
int learner_values(const char *fn, uavtrack_learner *learner, bool target, int64_t n, const float *rows, float *values,
                   void *stream)
{
    if (!learner) return fail("%s: null handle", fn);
    if (!rows || !values) return fail("%s: rows and values must not be null", fn);
    if (n < 1) return fail("%s: n = %lld < 1", fn, (long long)n);
    if (n > INT64_MAX / 48) return fail("%s: n = %lld rows overflow", fn, (long long)n);
    if (((uintptr_t)rows & 15) != 0) return fail("%s: rows must be 16-byte aligned", fn);
    if (target && !learner->d.target_mode) return fail("%s: no target critic is enabled (uavtrack_learner_set_target)", fn);
    ON_DEVICE(learner->cfg.device_id);
    HIP_TRY(launch_learner_values(learner->d, target, n, rows, values, static_cast<hipStream_t>(stream)));
    return 0;
}

// theta- <- the critic as it stands when the copy runs: uavtrack_learner_set_target (off -> on) and _sync_target
hipError_t copy_critic_to_target(const LearnerDevice &d, void *stream)
{
    return hipMemcpyAsync(d.target, d.params + d.L.c_w1, sizeof(float) * (size_t)learner_critic_words(d.L),
                          hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int uavtrack_learner_create(const uavtrack_learner_config *cfg, uavtrack_learner **out)
{
    auto check = [](const char *fn, const uavtrack_learner_config &c) {
        if (c.hidden < 1 || c.hidden > kLearnerMaxHidden)
            return fail("%s: hidden %d out of range [1, %d]", fn, c.hidden, kLearnerMaxHidden);
        if (c.n_actions < 1 || c.n_actions > kLearnerMaxActions)
            return fail("%s: n_actions %d out of range [1, %d]", fn, c.n_actions, kLearnerMaxActions);
        if (c.loss != UAVTRACK_LOSS_REFERENCE && c.loss != UAVTRACK_LOSS_PER_SAMPLE)
            return fail("%s: unknown loss form %d", fn, c.loss);
        if (c.max_batch < 0 || c.max_batch > kLearnerMaxBatch)
            return fail("%s: max_batch %lld out of range [0, %lld]", fn, (long long)c.max_batch, (long long)kLearnerMaxBatch);
        if (!std::isfinite(c.gamma) || !std::isfinite(c.actor_lr) || !std::isfinite(c.critic_lr) || c.actor_lr < 0 ||
            c.critic_lr < 0)
            return fail("%s: gamma and the learning rates must be finite, the rates >= 0", fn);
        return 0;
    };
    auto init = [](LearnerDevice &d, const uavtrack_learner_config &c) {
        d.L = LearnerLayout::make(c.hidden, c.n_actions);
        d.gamma = (float)c.gamma;
        d.actor_lr = (float)c.actor_lr;
        d.critic_lr = (float)c.critic_lr;
        d.per_sample = c.loss == UAVTRACK_LOSS_PER_SAMPLE;
        d.opt.tensors = kLearnerTensors;
        d.opt.P = d.L.P;
        d.max_n = c.max_batch ? c.max_batch : kLearnerDefaultBatch;
        d.max_norm[0] = d.max_norm[1] = INFINITY;       // regularisation off: entropy_coef 0, no diagnostics
        d.adv_eps = 1e-8;                               // the advantage raw
        return learner_prepare_kernels(d.L);
    };
    if (create_handle(__func__, cfg, out, check, init)) return 1;
    // the constant pair a stored advantage in raw mode goes through: x - 0 and x * 1 are exact
    const float unit[2] = {0.0f, 1.0f};
    DeviceGuard guard((*out)->cfg.device_id);
    const hipError_t e = hipMemcpy((*out)->d.adv_unit, unit, sizeof unit, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)uavtrack_learner_destroy(*out);
        *out = nullptr;
        return fail("%s: %s", __func__, hipGetErrorString(e));
    }
    return 0;
}

int uavtrack_learner_destroy(uavtrack_learner *learner)
{
    if (learner && learner->d.target) {
        DeviceGuard guard(learner->cfg.device_id);
        (void)hipDeviceSynchronize();
        release(target_bufs(learner->d));
    }
    return destroy_handle(learner);                 // (the TD and KL passes' scratch is in scratch_bufs() once it exists)
}

int uavtrack_learner_num_params(uavtrack_learner *learner, int64_t *out)
{
    if (!learner || !out) return fail("uavtrack_learner_num_params: null argument");
    *out = learner->d.L.P;
    return 0;
}

int uavtrack_learner_set_regularisation(uavtrack_learner *learner, double entropy_coef, double actor_max_norm,
                                        double critic_max_norm)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (!std::isfinite(entropy_coef) || entropy_coef < 0)
        return fail("%s: entropy_coef = %g must be finite and >= 0", __func__, entropy_coef);
    if (!(actor_max_norm > 0) || !(critic_max_norm > 0))
        return fail("%s: max norms (%g, %g) must be > 0, or +inf for no clipping", __func__, actor_max_norm, critic_max_norm);
    if (entropy_coef != 0 && !learner->d.per_sample)
        return fail("%s: entropy_coef = %g on a UAVTRACK_LOSS_REFERENCE learner: that form scales the actor's gradient "
                    "sums once by -mean(delta) / N, a factor an entropy term cannot share; use UAVTRACK_LOSS_PER_SAMPLE",
                    __func__, entropy_coef);
    learner->d.entropy_coef = (float)entropy_coef;
    learner->d.max_norm[0] = actor_max_norm;
    learner->d.max_norm[1] = critic_max_norm;
    learner->reg[0] = entropy_coef; learner->reg[1] = actor_max_norm; learner->reg[2] = critic_max_norm;
    return 0;
}

int uavtrack_learner_get_regularisation(uavtrack_learner *learner, double out[3])
{
    if (!learner || !out) return fail("%s: null argument", __func__);
    for (int k = 0; k < 3; ++k) out[k] = learner->reg[k];
    return 0;
}

int uavtrack_learner_set_diagnostics(uavtrack_learner *learner, float *entropy, int64_t capacity_rows, float *grad_norm)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (entropy && capacity_rows < 1)
        return fail("%s: capacity_rows = %lld < 1 with an entropy buffer", __func__, (long long)capacity_rows);
    learner->d.entropy = entropy;
    learner->d.entropy_rows = entropy ? capacity_rows : 0;
    learner->d.grad_norm = grad_norm;
    return 0;
}

int uavtrack_learner_reserve(uavtrack_learner *learner, int64_t max_batch)
{
    return reserve_scratch(__func__, learner, max_batch, kLearnerMaxBatch, &LearnerDevice::max_n);
}

int uavtrack_learner_set_params(uavtrack_learner *learner, const float *params, int64_t n_floats, void *stream)
{
    if (!learner || !params) return fail("uavtrack_learner_set_params: null argument");
    if (n_floats != learner->d.L.P)
        return fail("uavtrack_learner_set_params: %lld floats, the networks have %d", (long long)n_floats, learner->d.L.P);
    ON_DEVICE(learner->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpyAsync(learner->d.params, params, (size_t)n_floats * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int uavtrack_learner_get_params(uavtrack_learner *learner, float *params, int64_t n_floats, void *stream)
{
    if (!learner || !params) return fail("uavtrack_learner_get_params: null argument");
    if (n_floats != learner->d.L.P)
        return fail("uavtrack_learner_get_params: %lld floats, the networks have %d", (long long)n_floats, learner->d.L.P);
    ON_DEVICE(learner->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(params, learner->d.params, (size_t)n_floats * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int uavtrack_learner_publish_actor(uavtrack_learner *learner, uavtrack_env *env, void *stream)
{
    if (!learner || !env) return fail("uavtrack_learner_publish_actor: null handle");
    if (learner->cfg.device_id != env->cfg.device_id)
        return fail("uavtrack_learner_publish_actor: the learner is on device %d, the environment on device %d",
                    learner->cfg.device_id, env->cfg.device_id);
    const LearnerLayout &L = learner->d.L;
    const float *p = learner->d.params;
    return publish_actor(__func__, env, p + L.a_w1, p + L.a_b1, p + L.a_w2, p + L.a_b2, L.H, L.A, stream);
}

int uavtrack_learner_set_optimizer_state(uavtrack_learner *learner, const float *exp_avg, const float *exp_avg_sq,
                                         const int64_t *step, int64_t n_floats, void *stream)
{
    return optimizer_state(__func__, learner, exp_avg, exp_avg_sq, step, n_floats, stream, "the networks have %d");
}

int uavtrack_learner_get_optimizer_state(uavtrack_learner *learner, float *exp_avg, float *exp_avg_sq, int64_t *step,
                                         int64_t n_floats, void *stream)
{
    return optimizer_state(__func__, learner, exp_avg, exp_avg_sq, step, n_floats, stream, "the networks have %d");
}

int uavtrack_learner_update(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                            const float *rewards, const float *next_states, int64_t capacity, const int64_t *indices,
                            float *actor_loss, float *critic_loss, float *td_delta, float *priorities, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices};
    q.actor_loss = actor_loss; q.critic_loss = critic_loss; q.td_delta = td_delta; q.priorities = priorities;
    return run_learner_batch(__func__, learner, q, Batch::Update, nullptr, stream);
}

int uavtrack_learner_update_weighted(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                     const float *rewards, const float *next_states, int64_t capacity,
                                     const int64_t *indices, const float *weights, float *actor_loss, float *critic_loss,
                                     float *td_delta, float *priorities, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights};
    q.actor_loss = actor_loss; q.critic_loss = critic_loss; q.td_delta = td_delta; q.priorities = priorities;
    return run_learner_batch(__func__, learner, q, Batch::Update, nullptr, stream);
}

int uavtrack_learner_update_discounted(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                       const float *rewards, const float *next_states, int64_t capacity,
                                       const int64_t *indices, const float *weights, const float *discounts,
                                       float *actor_loss, float *critic_loss, float *td_delta, float *priorities,
                                       void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.actor_loss = actor_loss; q.critic_loss = critic_loss; q.td_delta = td_delta; q.priorities = priorities;
    return run_learner_batch(__func__, learner, q, Batch::Update, nullptr, stream);
}

int uavtrack_learner_update_clipped(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                    const float *rewards, const float *next_states, int64_t capacity,
                                    const int64_t *indices, const float *weights, const float *discounts,
                                    const float *log_mu, double clip_eps, float *ratio_out, float *actor_loss,
                                    float *critic_loss, float *td_delta, float *priorities, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.clipped = true; q.log_mu = log_mu; q.clip_eps = clip_eps; q.ratio = ratio_out;
    q.actor_loss = actor_loss; q.critic_loss = critic_loss; q.td_delta = td_delta; q.priorities = priorities;
    return run_learner_batch(__func__, learner, q, Batch::Update, nullptr, stream);
}

int uavtrack_learner_row_floats(uavtrack_learner *learner, int64_t *out)
{
    if (!learner || !out) return fail("uavtrack_learner_row_floats: null argument");
    *out = (int64_t)learner->d.L.P + kLearnerRowTail;
    return 0;
}

int uavtrack_learner_grad(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                          const float *rewards, const float *next_states, int64_t capacity, const int64_t *indices,
                          float *td_delta, float *row, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices};
    q.td_delta = td_delta;
    return run_learner_batch(__func__, learner, q, Batch::Grad, row, stream);
}

int uavtrack_learner_grad_weighted(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                   const float *rewards, const float *next_states, int64_t capacity,
                                   const int64_t *indices, const float *weights, float *td_delta, float *row, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights};
    q.td_delta = td_delta;
    return run_learner_batch(__func__, learner, q, Batch::Grad, row, stream);
}

int uavtrack_learner_grad_discounted(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                     const float *rewards, const float *next_states, int64_t capacity,
                                     const int64_t *indices, const float *weights, const float *discounts, float *td_delta,
                                     float *row, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.td_delta = td_delta;
    return run_learner_batch(__func__, learner, q, Batch::Grad, row, stream);
}

int uavtrack_learner_grad_clipped(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                  const float *rewards, const float *next_states, int64_t capacity, const int64_t *indices,
                                  const float *weights, const float *discounts, const float *log_mu, double clip_eps,
                                  float *ratio_out, float *td_delta, float *row, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.clipped = true; q.log_mu = log_mu; q.clip_eps = clip_eps; q.ratio = ratio_out;
    q.td_delta = td_delta;
    return run_learner_batch(__func__, learner, q, Batch::Grad, row, stream);
}

int uavtrack_learner_update_stored(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                   const float *rewards, const float *next_states, int64_t capacity,
                                   const int64_t *indices, const float *weights, const float *discounts,
                                   const float *advantages, const float *log_mu, double clip_eps, float *ratio_out,
                                   float *actor_loss, float *critic_loss, float *td_delta, float *priorities, void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.stored = true; q.advantages = advantages;
    q.log_mu = log_mu; q.clip_eps = clip_eps; q.ratio = log_mu ? ratio_out : nullptr;
    q.actor_loss = actor_loss; q.critic_loss = critic_loss; q.td_delta = td_delta; q.priorities = priorities;
    return run_learner_batch(__func__, learner, q, Batch::Update, nullptr, stream);
}

int uavtrack_learner_grad_stored(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                 const float *rewards, const float *next_states, int64_t capacity, const int64_t *indices,
                                 const float *weights, const float *discounts, const float *advantages,
                                 const float *log_mu, double clip_eps, float *ratio_out, float *td_delta, float *row,
                                 void *stream)
{
    LearnerLaunch q = {n, capacity, states, rewards, next_states, actions, indices, weights, discounts};
    q.stored = true; q.advantages = advantages;
    q.log_mu = log_mu; q.clip_eps = clip_eps; q.ratio = log_mu ? ratio_out : nullptr;
    q.td_delta = td_delta;
    return run_learner_batch(__func__, learner, q, Batch::Grad, row, stream);
}

int uavtrack_learner_apply(uavtrack_learner *learner, const float *rows, int64_t count, float *actor_loss,
                           float *critic_loss, void *stream)
{
    if (!learner) return fail("uavtrack_learner_apply: null handle");
    if (!rows) return fail("uavtrack_learner_apply: rows must not be null");
    if (!actor_loss || !critic_loss) return fail("uavtrack_learner_apply: actor_loss and critic_loss must not be null");
    if (count < 1 || count > UAVTRACK_LEARNER_MAX_ROWS)
        return fail("uavtrack_learner_apply: count = %lld out of range [1, %d]", (long long)count, UAVTRACK_LEARNER_MAX_ROWS);
    if (learner->d.kl_on)
        return fail("uavtrack_learner_apply: KL early stopping is on (uavtrack_learner_set_kl_stop): gradient rows carry "
                    "no KL sum, so the split update is refused; turn the stop off");
    ON_DEVICE(learner->cfg.device_id);
    HIP_TRY(launch_learner_apply(learner->d, rows, (int)count, actor_loss, critic_loss, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_learner_write_priorities(uavtrack_learner *learner, int64_t n, const int64_t *indices, int64_t capacity,
                                      const float *td_delta, float *priorities, void *stream)
{
    if (!learner) return fail("uavtrack_learner_write_priorities: null handle");
    if (!td_delta || !priorities) return fail("uavtrack_learner_write_priorities: td_delta and priorities must not be null");
    if (accept_batch(__func__, learner, n, capacity, indices, "into")) return 1;
    ON_DEVICE(learner->cfg.device_id);
    HIP_TRY(launch_learner_priorities(learner->d, indices, n, capacity, td_delta, priorities,
                                      static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_learner_values(uavtrack_learner *learner, int64_t n, const float *rows, float *values, void *stream)
{
    return learner_values(__func__, learner, false, n, rows, values, stream);
}

// ---- the normalised advantage

int uavtrack_learner_set_advantage(uavtrack_learner *learner, int32_t mode, double eps, const float *given)
{
    static_assert(UAVTRACK_ADVANTAGE_RAW == kAdvantageRaw && UAVTRACK_ADVANTAGE_BATCH == kAdvantageBatch &&
                  UAVTRACK_ADVANTAGE_GIVEN == kAdvantageGiven, "learner.h restates enum uavtrack_advantage_mode");
    if (!learner) return fail("%s: null handle", __func__);
    if (mode != UAVTRACK_ADVANTAGE_RAW && mode != UAVTRACK_ADVANTAGE_BATCH && mode != UAVTRACK_ADVANTAGE_GIVEN)
        return fail("%s: unknown mode %d", __func__, mode);
    if (!(eps >= 0)) return fail("%s: eps = %g must be >= 0", __func__, eps);
    if (mode == UAVTRACK_ADVANTAGE_GIVEN && !given)
        return fail("%s: UAVTRACK_ADVANTAGE_GIVEN needs the {mean, inv_std} pair: given must not be null", __func__);
    LearnerDevice &d = learner->d;
    if (mode != UAVTRACK_ADVANTAGE_RAW && !d.per_sample)
        return fail("%s: a normalised advantage on a UAVTRACK_LOSS_REFERENCE learner: that form scales the actor's gradient "
                    "sums once by -mean(delta) / N, and a standardised advantage has mean 0; use UAVTRACK_LOSS_PER_SAMPLE",
                    __func__);
    if (mode == UAVTRACK_ADVANTAGE_BATCH && !d.adv_td) {
        // the TD pass's scratch, once per handle at the reserved size (uavtrack_learner_reserve grows it with the rest)
        ON_DEVICE(learner->cfg.device_id);
        HIP_TRY(replace(advantage_bufs(d, d.max_n)));
    }
    d.adv_mode = mode;
    d.adv_eps = eps;
    d.adv_given = mode == UAVTRACK_ADVANTAGE_GIVEN ? given : nullptr;
    return 0;
}

int uavtrack_learner_get_advantage(uavtrack_learner *learner, int32_t *mode, double *eps, const float **given)
{
    if (!learner || !mode || !eps || !given) return fail("%s: null argument", __func__);
    *mode = learner->d.adv_mode; *eps = learner->d.adv_eps; *given = learner->d.adv_given;
    return 0;
}

int uavtrack_learner_set_advantage_stats(uavtrack_learner *learner, float *stats)
{
    if (!learner) return fail("%s: null handle", __func__);
    learner->d.adv_user = stats;
    return 0;
}

// ---- KL early stopping

int uavtrack_learner_set_kl_stop(uavtrack_learner *learner, int32_t on, double limit, float *kl_out, int32_t *state)
{
    if (!learner) return fail("%s: null handle", __func__);
    LearnerDevice &d = learner->d;
    if (!on) {
        d.kl_on = 0; d.kl_limit = INFINITY; d.kl_out = nullptr; d.kl_state = nullptr;
        learner->kl_limit = INFINITY;
        return 0;
    }
    if (!(limit >= 0)) return fail("%s: limit = %g must be >= 0 (+inf: observe, never stop)", __func__, limit);
    if (!kl_out || !state) return fail("%s: kl_out and state must not be null while on", __func__);
    if (!d.per_sample)
        return fail("%s: KL early stopping on a UAVTRACK_LOSS_REFERENCE learner: the estimate is formed from the clipped "
                    "surrogate's ratios, which that form does not have; use UAVTRACK_LOSS_PER_SAMPLE", __func__);
    if (!d.kl_ratio) {
        // the KL pass's scratch, once per handle at the reserved size (uavtrack_learner_reserve grows it with the rest)
        ON_DEVICE(learner->cfg.device_id);
        HIP_TRY(replace(kl_bufs(d, d.max_n)));
    }
    d.kl_on = 1; d.kl_limit = (float)limit; d.kl_out = kl_out; d.kl_state = state;
    learner->kl_limit = limit;
    return 0;
}

int uavtrack_learner_get_kl_stop(uavtrack_learner *learner, int32_t *on, double *limit, float **kl_out, int32_t **state)
{
    if (!learner || !on || !limit || !kl_out || !state) return fail("%s: null argument", __func__);
    *on = learner->d.kl_on; *limit = learner->kl_limit; *kl_out = learner->d.kl_out; *state = learner->d.kl_state;
    return 0;
}

int uavtrack_learner_kl_reset(uavtrack_learner *learner, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (!learner->d.kl_on) return fail("%s: KL early stopping is off (uavtrack_learner_set_kl_stop)", __func__);
    ON_DEVICE(learner->cfg.device_id);
    HIP_TRY(launch_learner_kl_reset(learner->d, static_cast<hipStream_t>(stream)));
    return 0;
}

// ---- the target critic

int uavtrack_learner_set_target(uavtrack_learner *learner, int32_t mode, double tau, int64_t period, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (mode != UAVTRACK_TARGET_OFF && mode != UAVTRACK_TARGET_POLYAK && mode != UAVTRACK_TARGET_PERIODIC)
        return fail("%s: unknown mode %d", __func__, mode);
    if (mode == UAVTRACK_TARGET_POLYAK && !(tau > 0 && tau <= 1))
        return fail("%s: tau = %g must lie in (0, 1]", __func__, tau);
    if (mode == UAVTRACK_TARGET_PERIODIC && period < 1) return fail("%s: period = %lld < 1", __func__, (long long)period);
    LearnerDevice &d = learner->d;
    if (mode != UAVTRACK_TARGET_OFF && !d.target_mode) {
        // off -> on: the block (once per handle), then a hard copy of the critic as it stands, stream-ordered
        ON_DEVICE(learner->cfg.device_id);
        if (!d.target) HIP_TRY(replace(target_bufs(d)));
        HIP_TRY(copy_critic_to_target(d, stream));
    }
    d.target_mode = mode;
    d.target_tau = mode == UAVTRACK_TARGET_POLYAK ? (float)tau : 0.0f;
    d.target_omt = 1.0f - d.target_tau;
    d.target_period = mode == UAVTRACK_TARGET_PERIODIC ? period : 0;
    learner->target_tau = mode == UAVTRACK_TARGET_POLYAK ? tau : 0.0;
    return 0;
}

int uavtrack_learner_get_target(uavtrack_learner *learner, double out[3])
{
    if (!learner || !out) return fail("%s: null argument", __func__);
    out[0] = learner->d.target_mode; out[1] = learner->target_tau; out[2] = (double)learner->d.target_period;
    return 0;
}

int uavtrack_learner_sync_target(uavtrack_learner *learner, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    const LearnerDevice &d = learner->d;
    if (!d.target_mode) return fail("%s: no target critic is enabled (uavtrack_learner_set_target)", __func__);
    ON_DEVICE(learner->cfg.device_id);
    HIP_TRY(copy_critic_to_target(d, stream));
    return 0;
}

}  // extern "C"

namespace {

// uavtrack_learner_set_target_params / _get_target_params: P = const float (in from the host) or float (out to it)
template <typename P>
int target_params(const char *fn, uavtrack_learner *learner, P *params, int64_t n_floats, void *stream)
{
    if (!learner || !params) return fail("%s: null argument", fn);
    const LearnerDevice &d = learner->d;
    if (!d.target_mode) return fail("%s: no target critic is enabled (uavtrack_learner_set_target)", fn);
    if (n_floats != learner_critic_words(d.L))
        return fail("%s: %lld floats, the critic has %d", fn, (long long)n_floats, learner_critic_words(d.L));
    ON_DEVICE(learner->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if constexpr (std::is_const<P>::value) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpyAsync(d.target, params, (size_t)n_floats * 4, hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(hipMemcpyAsync(params, d.target, (size_t)n_floats * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int uavtrack_learner_set_target_params(uavtrack_learner *learner, const float *params, int64_t n_floats, void *stream)
{
    return target_params(__func__, learner, params, n_floats, stream);
}

int uavtrack_learner_get_target_params(uavtrack_learner *learner, float *params, int64_t n_floats, void *stream)
{
    return target_params(__func__, learner, params, n_floats, stream);
}

int uavtrack_learner_values_target(uavtrack_learner *learner, int64_t n, const float *rows, float *values, void *stream)
{
    return learner_values(__func__, learner, true, n, rows, values, stream);
}

}  // extern "C"

namespace {

// what uavtrack_learner_log_probs, _log_probs_window and _ratio_weights test alike, after their null tests
int accept_policy_rows(const char *fn, int64_t n, const float *states, int64_t capacity)
{
    if (n < 1) return fail("%s: n = %lld < 1", fn, (long long)n);
    if (capacity < 1) return fail("%s: capacity = %lld < 1", fn, (long long)capacity);
    if (capacity > INT64_MAX / 48) return fail("%s: capacity = %lld slots overflow", fn, (long long)capacity);
    if (((uintptr_t)states & 15) != 0) return fail("%s: states must be 16-byte aligned", fn);
    return 0;
}

PolicyLaunch policy_rows(int64_t n, const float *states, const int32_t *actions, int64_t capacity, const int64_t *indices)
{
    PolicyLaunch q = {};
    q.n = n; q.capacity = capacity; q.first = -1; q.states = states; q.actions = actions; q.idx = indices;
    return q;
}

}  // namespace

extern "C" {

int uavtrack_learner_log_probs(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                               int64_t capacity, const int64_t *indices, float *log_probs, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (!states || !actions || !log_probs) return fail("%s: states, actions and log_probs must not be null", __func__);
    if (accept_policy_rows(__func__, n, states, capacity)) return 1;
    if (!indices && n > capacity)
        return fail("%s: n = %lld rows without indices from a store of %lld", __func__, (long long)n, (long long)capacity);
    ON_DEVICE(learner->cfg.device_id);
    PolicyLaunch q = policy_rows(n, states, actions, capacity, indices);
    q.log_probs = log_probs;
    HIP_TRY(launch_learner_policy(learner->d, q, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_learner_log_probs_window(uavtrack_learner *learner, const float *states, const int32_t *actions,
                                      int64_t capacity, int64_t first, int64_t n, float *log_mu, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (!states || !actions || !log_mu) return fail("%s: states, actions and log_mu must not be null", __func__);
    if (accept_policy_rows(__func__, n, states, capacity)) return 1;
    if (n > capacity) return fail("%s: a window of n = %lld slots in a ring of %lld", __func__, (long long)n, (long long)capacity);
    if (first < 0 || first >= capacity)
        return fail("%s: first = %lld outside [0, %lld)", __func__, (long long)first, (long long)capacity);
    ON_DEVICE(learner->cfg.device_id);
    PolicyLaunch q = policy_rows(n, states, actions, capacity, nullptr);
    q.first = first;
    q.log_probs = log_mu;
    HIP_TRY(launch_learner_policy(learner->d, q, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_learner_ratio_weights(uavtrack_learner *learner, int64_t n, const float *states, const int32_t *actions,
                                   const float *log_mu, int64_t capacity, const int64_t *indices, double rho_bar,
                                   const float *weights_in, float *weights_out, float *rho_out, void *stream)
{
    if (!learner) return fail("%s: null handle", __func__);
    if (!states || !actions || !log_mu || !weights_out)
        return fail("%s: states, actions, log_mu and weights_out must not be null", __func__);
    if (accept_policy_rows(__func__, n, states, capacity)) return 1;
    if (!indices && n > capacity)
        return fail("%s: n = %lld rows without indices from a store of %lld", __func__, (long long)n, (long long)capacity);
    if (!(rho_bar > 0)) return fail("%s: rho_bar = %g must be > 0 (+inf: untruncated)", __func__, rho_bar);
    ON_DEVICE(learner->cfg.device_id);
    PolicyLaunch q = policy_rows(n, states, actions, capacity, indices);
    q.log_mu = log_mu; q.rho_bar = (float)rho_bar; q.weights_in = weights_in; q.weights_out = weights_out; q.rho_out = rho_out;
    HIP_TRY(launch_learner_policy(learner->d, q, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_learner_check(uavtrack_learner *learner, int64_t *refused, void *stream)
{
    int count = 0;
    if (take_refusals(__func__, learner, refused, stream, &count)) return 1;
    if (count)
        return fail("uavtrack_learner_check: %d update(s) refused: an action outside [0, %d), an index outside "
                    "[0, capacity), an importance weight that is NaN, infinite or negative, a discount that is NaN or "
                    "outside [0, 1], a behaviour log-probability that is NaN or positive or a ratio that is not finite "
                    "(the clipped surrogate), a given advantage mean that is not finite or inv_std that is NaN, infinite or "
                    "negative, a stored advantage that is NaN or infinite, or (uavtrack_learner_apply) a gradient row of another "
                    "layout; they changed nothing",
                    count, learner->d.L.A);
    return 0;
}

}  // extern "C"

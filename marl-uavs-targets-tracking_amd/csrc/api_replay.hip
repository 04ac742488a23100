// api_replay.hip -- the C ABI of the replay ring (include/uavtrack.h, uavtrack_replay_*).

#include "api_handle.h"
#include "replay.h"

#include <cmath>

using namespace uavtrack;

struct uavtrack_replay {
    uavtrack_replay_config cfg;
    ReplayDevice d;
};

namespace uavtrack {

static Bufs device_bufs(ReplayDevice &d)
{
    const size_t tiles = (size_t)((d.max_capacity + kReplayTile - 1) / kReplayTile);
    return {buf(d.prefix, tiles), buf(d.tile_last, tiles), buf(d.counter, 2, true), buf(d.pmin, 1),
            buf(d.pdraw, (size_t)d.max_batch), buf(d.parts, kReplayMaxParts + 1), buf(d.status, 1, true),
            buf(d.errors, 1, true)};
}

static int *refusal_word(const ReplayDevice &d) { return d.errors; }

}  // namespace uavtrack

namespace {

constexpr int64_t kReplayMaxBatch = ((int64_t)1 << 31) - 1;   // draw numbers are Philox counter word 0
constexpr int64_t kReplayMaxCapacity = (int64_t)kReplayTile * ((int64_t)1 << 30);   // tile numbers are int32

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The ring's pointers and host state against the handle's limits (`fn` names the ABI function in the message).  The
// adds need the stores and take a ring without priorities (a uniform ring); the prioritised draws need the priorities.
int accept_ring(const uavtrack_replay *r, const char *fn, const uavtrack_replay_ring *ring, bool stores, bool priorities)
{
    if (!ring) return fail("%s: ring is null", fn);
    if (priorities && !ring->priorities) return fail("%s: ring->priorities is null", fn);
    if (stores && (!ring->states || !ring->actions || !ring->rewards || !ring->next_states))
        return fail("%s: the ring's states, actions, rewards and next_states must not be null", fn);
    if (stores && (!aligned16(ring->states) || !aligned16(ring->next_states)))
        return fail("%s: the ring's states and next_states must be 16-byte aligned", fn);
    if (ring->capacity < 1 || ring->capacity > r->cfg.max_capacity)
        return fail("%s: capacity %lld outside [1, max_capacity = %lld]", fn, (long long)ring->capacity,
                    (long long)r->cfg.max_capacity);
    if (ring->count < 0 || ring->count > ring->capacity)
        return fail("%s: count %lld outside [0, capacity = %lld]", fn, (long long)ring->count, (long long)ring->capacity);
    if (ring->pos < 0 || ring->pos >= ring->capacity)
        return fail("%s: pos %lld outside [0, capacity = %lld)", fn, (long long)ring->pos, (long long)ring->capacity);
    return 0;
}

ReplayRingView ring_view(const uavtrack_replay_ring *ring)
{
    ReplayRingView v;
    v.states = ring->states; v.actions = ring->actions; v.rewards = ring->rewards; v.next_states = ring->next_states;
    v.priorities = ring->priorities; v.capacity = ring->capacity; v.pos = ring->pos; v.count = ring->count;
    return v;
}

// One request to add to a ring, as each of the six add entry points states it: the launcher's own request plus what
// only the acceptor needs.  The flat form is one step of n "environments"; uavtrack_replay_add_rollout knows only
// agents = envs * n_uav, and passes it as envs.
struct ReplayAddCall {
    const char *who;                   // the entry point, as the error messages name it
    const uavtrack_replay_ring *ring;  // (a.ring is filled once this one is accepted)
    bool episodes = false;             // the entry point has done / start_obs: _episodes requires them, the n-step and
                                       // lambda forms and the GAE form take both or neither
    double lambda = 0.0, gamma = 0.0;  // as given: checked as doubles, launched as floats
    ReplayAdd a{};

    ReplayAddCall(const char *who_, const uavtrack_replay_ring *ring_, ReplayForm form, int64_t steps, int64_t envs,
                  int64_t n_uav, const float *obs_in, const float *next, const int32_t *actions, const float *rewards)
        : who(who_), ring(ring_)
    {
        a.form = form; a.steps = steps; a.envs = envs; a.n_uav = n_uav; a.n_step = 1;
        a.obs_in = obs_in; a.next = next; a.actions = actions; a.rewards = rewards;
    }
};

// Every refusal of the add entry points, in one order.  Nothing has been enqueued when one of them fires.
int accept_replay_add(const uavtrack_replay *replay, const ReplayAddCall &q)
{
    const char *who = q.who;
    const ReplayAdd &a = q.a;
    if (!replay) return fail("%s: null handle", who);
    if (accept_ring(replay, who, q.ring, true, false)) return 1;
    const bool flat = a.form == ReplayForm::Flat, plain = a.form == ReplayForm::Rollout, lambda = a.form == ReplayForm::Lambda;
    const bool given = (flat ? a.states : a.obs_in) && a.next && a.actions && a.rewards;
    if (!given || (!flat && !plain && !a.discounts) || (plain && q.episodes && (!a.done || !a.start_obs)) || (lambda && !a.values))
        return fail("%s: %s must not be null", who,
                    flat ? "states, actions, rewards and next_states"
                    : lambda ? "discounts, obs_in, obs, actions, reward and values"
                    : !plain ? "discounts, obs_in, obs, actions and reward"
                    : q.episodes ? "obs_in, obs, actions, reward, done and start_obs" : "obs_in, obs, actions and reward");
    if (a.form == ReplayForm::Gae && (!a.values || !a.values_in || !a.advantages))
        return fail("%s: advantages, values and values_in must not be null", who);
    if (!a.done != !a.start_obs) return fail("%s: done and start_obs must both be given or both be null", who);
    if (a.form == ReplayForm::Gae && !a.done != !a.values_start)
        return fail("%s: values_start comes with done and start_obs: all three given or all three null", who);
    if (!aligned16(flat ? a.states : a.obs_in) || !aligned16(a.next) || !aligned16(a.start_obs))
        return fail("%s: %s must be 16-byte aligned", who,
                    flat ? "states and next_states" : q.episodes ? "obs_in, obs and start_obs" : "obs_in and obs");
    if (a.n_step < 1 || a.n_step > UAVTRACK_REPLAY_MAX_NSTEP)
        return fail("%s: n_step = %d outside [1, %d]", who, a.n_step, UAVTRACK_REPLAY_MAX_NSTEP);
    if (!(q.lambda >= 0.0 && q.lambda <= 1.0)) return fail("%s: lambda = %g is not a finite value in [0, 1]", who, q.lambda);
    if (!(q.gamma >= 0.0 && q.gamma <= 1.0)) return fail("%s: gamma = %g is not a finite value in [0, 1]", who, q.gamma);
    if (flat) return a.steps < 1 ? fail("%s: n = %lld < 1", who, (long long)a.steps) : 0;   // (no product is taken of n)
    if (a.steps < 1 || a.envs < 1 || a.n_uav < 1)
        return fail("%s: %s must be >= 1", who, q.episodes ? "steps, envs and n_uav" : "steps and agents");
    if (a.envs > INT64_MAX / a.n_uav || a.steps > INT64_MAX / (a.envs * a.n_uav) / 12)
        return fail("%s: %s overflows", who, q.episodes ? "steps * envs * n_uav" : "steps * agents");
    return 0;
}

int run_replay_add(uavtrack_replay *replay, const ReplayAddCall &q, void *stream)
{
    if (accept_replay_add(replay, q)) return 1;
    ReplayAdd a = q.a;
    a.ring = ring_view(q.ring); a.lambda = (float)q.lambda; a.gamma = (float)q.gamma;
    ON_DEVICE(replay->cfg.device_id);
    HIP_TRY(launch_replay_add(replay->d, a, static_cast<hipStream_t>(stream)));
    return 0;
}

// What the three draws refuse alike: the handle, the ring (with its priorities for the prioritised draws), indices, n
// and an empty ring.
int accept_draw(const uavtrack_replay *replay, const char *fn, const uavtrack_replay_ring *ring, bool priorities, int64_t n,
                const int64_t *indices)
{
    if (!replay) return fail("%s: null handle", fn);
    if (accept_ring(replay, fn, ring, false, priorities)) return 1;
    if (!indices) return fail("%s: indices must not be null", fn);
    if (n < 1 || n > replay->cfg.max_batch)
        return fail("%s: n = %lld outside [1, max_batch = %lld]", fn, (long long)n, (long long)replay->cfg.max_batch);
    if (ring->count < 1) return fail("%s: the ring is empty (count = 0)", fn);
    return 0;
}

// uavtrack_replay_sample (anneal_calls == 0: beta0 is the call's beta) and _sample_annealed (anneal_calls >= 1)
int replay_sample(const char *fn, uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, double alpha,
                  double beta0, double beta1, int64_t anneal_calls, int64_t *indices, float *weights, void *stream)
{
    if (accept_draw(replay, fn, ring, true, n, indices)) return 1;
    if (!std::isfinite(alpha) || !(alpha > 0) || (float)alpha <= 0.0f)
        return fail("%s: alpha = %g must be finite and > 0", fn, alpha);
    const char *first = anneal_calls ? "beta0" : "beta";
    if (!std::isfinite(beta0) || !(beta0 >= 0)) return fail("%s: %s = %g must be finite and >= 0", fn, first, beta0);
    if (!std::isfinite(beta1) || !(beta1 >= 0)) return fail("%s: beta1 = %g must be finite and >= 0", fn, beta1);
    ON_DEVICE(replay->cfg.device_id);
    HIP_TRY(launch_replay_sample(replay->d, ring->priorities, ring->count, n, (float)alpha, beta0, beta1, anneal_calls,
                                 indices, weights, static_cast<hipStream_t>(stream)));
    return 0;
}

}  // namespace

extern "C" {

int uavtrack_replay_create(const uavtrack_replay_config *cfg, uavtrack_replay **out)
{
    auto check = [](const char *fn, const uavtrack_replay_config &c) {
        if (c.max_capacity < 1 || c.max_capacity > kReplayMaxCapacity)
            return fail("%s: max_capacity %lld out of range [1, %lld]", fn, (long long)c.max_capacity,
                        (long long)kReplayMaxCapacity);
        if (c.max_batch < 1 || c.max_batch > kReplayMaxBatch)
            return fail("%s: max_batch %lld out of range [1, %lld]", fn, (long long)c.max_batch, (long long)kReplayMaxBatch);
        return 0;
    };
    auto init = [](ReplayDevice &d, const uavtrack_replay_config &c) {
        d.max_capacity = c.max_capacity;
        d.max_batch = c.max_batch;
        d.k0 = (uint32_t)c.seed;
        d.k1 = (uint32_t)(c.seed >> 32);
        return hipSuccess;
    };
    return create_handle(__func__, cfg, out, check, init);
}

int uavtrack_replay_destroy(uavtrack_replay *replay) { return destroy_handle(replay); }

int uavtrack_replay_add(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, const float *states,
                        const int32_t *actions, const float *rewards, const float *next_states, void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Flat, n, 1, 1, nullptr, next_states, actions, rewards);
    q.a.states = states;
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_add_rollout(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t steps, int64_t agents,
                                const float *obs_in, const float *obs, const int32_t *actions, const float *reward,
                                void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Rollout, steps, agents, 1, obs_in, obs, actions, reward);
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_add_rollout_episodes(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t steps,
                                         int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                         const int32_t *actions, const float *reward, const uint8_t *done,
                                         const float *start_obs, void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Rollout, steps, envs, n_uav, obs_in, obs, actions, reward);
    q.episodes = true; q.a.done = done; q.a.start_obs = start_obs;
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_add_rollout_nstep(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                      int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                      const int32_t *actions, const float *reward, const uint8_t *done,
                                      const float *start_obs, int32_t n_step, double gamma, void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Nstep, steps, envs, n_uav, obs_in, obs, actions, reward);
    q.episodes = true; q.a.done = done; q.a.start_obs = start_obs;
    q.a.discounts = discounts; q.a.n_step = n_step; q.gamma = gamma;
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_add_rollout_lambda(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                       int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in, const float *obs,
                                       const int32_t *actions, const float *reward, const uint8_t *done,
                                       const float *start_obs, const float *values, double lambda, double gamma,
                                       void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Lambda, steps, envs, n_uav, obs_in, obs, actions, reward);
    q.episodes = true; q.a.done = done; q.a.start_obs = start_obs;
    q.a.discounts = discounts; q.a.values = values; q.lambda = lambda; q.gamma = gamma;
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_add_rollout_gae(uavtrack_replay *replay, const uavtrack_replay_ring *ring, float *discounts,
                                    float *advantages, int64_t steps, int64_t envs, int64_t n_uav, const float *obs_in,
                                    const float *obs, const int32_t *actions, const float *reward, const uint8_t *done,
                                    const float *start_obs, const float *values, const float *values_in,
                                    const float *values_start, double lambda, double gamma, void *stream)
{
    ReplayAddCall q(__func__, ring, ReplayForm::Gae, steps, envs, n_uav, obs_in, obs, actions, reward);
    q.episodes = true; q.a.done = done; q.a.start_obs = start_obs;
    q.a.discounts = discounts; q.a.values = values; q.lambda = lambda; q.gamma = gamma;
    q.a.advantages = advantages; q.a.values_in = values_in; q.a.values_start = values_start;
    return run_replay_add(replay, q, stream);
}

int uavtrack_replay_sample(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, double alpha,
                           double beta, int64_t *indices, float *weights, void *stream)
{
    return replay_sample(__func__, replay, ring, n, alpha, beta, beta, 0, indices, weights, stream);
}

int uavtrack_replay_sample_annealed(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, double alpha,
                                    double beta0, double beta1, int64_t anneal_calls, int64_t *indices, float *weights,
                                    void *stream)
{
    if (!replay) return fail("uavtrack_replay_sample_annealed: null handle");
    if (anneal_calls < 1) return fail("uavtrack_replay_sample_annealed: anneal_calls = %lld < 1", (long long)anneal_calls);
    return replay_sample(__func__, replay, ring, n, alpha, beta0, beta1, anneal_calls, indices, weights, stream);
}

int uavtrack_replay_sample_uniform(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t n, int64_t *indices,
                                   void *stream)
{
    if (accept_draw(replay, __func__, ring, false, n, indices)) return 1;
    if (n > ring->count)
        return fail("%s: n = %lld exceeds count = %lld (the draw is without replacement)", __func__, (long long)n,
                    (long long)ring->count);
    ON_DEVICE(replay->cfg.device_id);
    HIP_TRY(launch_replay_sample_uniform(replay->d, ring->count, n, indices, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_replay_sample_sweep(uavtrack_replay *replay, const uavtrack_replay_ring *ring, int64_t first, int64_t length,
                                 int64_t n, uint64_t *cursor, int64_t *indices, void *stream)
{
    if (accept_draw(replay, __func__, ring, false, n, indices)) return 1;
    if (!cursor) return fail("%s: cursor must not be null", __func__);
    if (length < 1) return fail("%s: length = %lld < 1", __func__, (long long)length);
    if (first < 0 || first >= ring->capacity)
        return fail("%s: first = %lld outside [0, capacity = %lld)", __func__, (long long)first, (long long)ring->capacity);
    if (n > length)
        return fail("%s: n = %lld exceeds length = %lld (a minibatch is part of the window)", __func__, (long long)n,
                    (long long)length);
    // the valid slots are [0, count), a circle once the ring is full (length > count, written so that nothing overflows)
    if (length > ring->count || (ring->count < ring->capacity && first > ring->count - length))
        return fail("%s: the window [%lld, %lld + %lld) leaves the ring's %lld valid slots (capacity %lld)", __func__,
                    (long long)first, (long long)first, (long long)length, (long long)ring->count,
                    (long long)ring->capacity);
    ON_DEVICE(replay->cfg.device_id);
    HIP_TRY(launch_replay_sample_sweep(replay->d, ring->capacity, first, length, n, cursor, indices,
                                       static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_replay_check(uavtrack_replay *replay, int64_t *refused, void *stream)
{
    int count = 0;
    if (take_refusals(__func__, replay, refused, stream, &count)) return 1;
    if (count)
        return fail("uavtrack_replay_check: %d sample call(s) refused: a priority in [0, count) is NaN, infinite or "
                    "negative, or all of them are zero; their indices are slot 0", count);
    return 0;
}

}  // extern "C"

// replay.h -- the replay ring (uavtrack_replay_*): what replay_kernel.hip and api_replay.hip share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uavtrack.h"

namespace uavtrack {

// replay_kernel.hip -- the prioritised replay ring (uavtrack_replay_*).  The ring's stores and priorities belong to the
// caller; the handle owns the scratch below.  Sampling works on tiles of kReplayTile slots: per-tile fp64 sums, one
// inclusive scan of them, then one wavefront per draw (binary search over the tile prefix, rescan of one tile).
constexpr int kReplayTile = 2048;
constexpr int kReplayMaxParts = 1024;         // workgroups of the priority-maximum reduction
constexpr uint32_t kReplayDomain = 0x52504C59u;   // "RPLY": Philox counter word 3 of the draw stream
constexpr uint32_t kUniformDomain = 0x554E4946u;  // "UNIF": Philox counter word 3 of the uniform draw's round keys
constexpr uint32_t kSweepDomain = 0x53574550u;    // "SWEP": Philox counter word 3 of the sweep's round keys
constexpr int kUniformRounds = 16;            // Feistel rounds of the uniform draw's and the sweep's bijection (four Philox
                                              // blocks of keys)
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
// Minibatch cursor[0] % (length / n) of epoch cursor[0] / (length / n) of a sweep over the window first, first + 1, ...
// (mod capacity) of `length` slots: n of them, no slot twice within an epoch.  cursor (DEVICE, 2 words, the caller's)
// is advanced on the device; the handle's call counter is neither read nor advanced.
hipError_t launch_replay_sample_sweep(const ReplayDevice &d, int64_t capacity, int64_t first, int64_t length, int64_t n,
                                      uint64_t *cursor, int64_t *indices, hipStream_t stream);
// One ring add of steps x envs x n_uav transitions, of which the last min(n, capacity) land in the ring from ring.pos on;
// ring.priorities == nullptr (a uniform ring): the stores alone.
//   Flat     states / next [n][12], actions / rewards [n], with steps = n and envs = n_uav = 1;
//   Rollout  obs_in [agents][12], next = obs [steps][agents][12], actions / rewards [steps][agents]; with done [steps][envs]
//            and start_obs (of obs's shape) the rollout crossed episode ends, without them envs * n_uav is just `agents`;
//   Nstep    Rollout's source folded into n_step-step returns with gamma; discounts [capacity] receives gamma^m per slot;
//   Lambda   Rollout's write, then the backward scan over each agent's chain that overwrites the written slots' rewards
//            with R_t and leaves d_t in discounts; values [steps][agents];
//   Gae      Lambda's write and fold, the scan storing G_t as the reward, +0 as the discount and G_t - V(s_t) in
//            advantages [capacity]; values_in [agents], values_start [steps][agents] (with done, else nullptr).
enum class ReplayForm { Flat, Rollout, Nstep, Lambda, Gae };
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
    float *advantages;              // the GAE form's alone, as are the two below
    const float *values_in, *values_start;
};
hipError_t launch_replay_add(const ReplayDevice &d, const ReplayAdd &q, hipStream_t stream);

}  // namespace uavtrack

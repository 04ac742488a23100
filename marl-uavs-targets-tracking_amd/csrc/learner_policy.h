// learner_policy.h -- the actor alone (uavtrack_learner_log_probs, _log_probs_window, _ratio_weights): what
// learner_policy_kernel.hip and api_learner.hip share.  Reaches learner.h for the learner's device state and layout, and
// nothing of the environment.
#pragma once

#include "learner.h"

namespace uavtrack {

// One launch of learner_policy_kernel.  Row i of n reads slot src_i = (first + i) % capacity when first >= 0 (a ring
// window), else idx[i] (idx null: i).  log p_i = log pi(actions[src_i] | states[src_i]) with the actor as it stands when
// the launch executes; NaN for a slot outside [0, capacity) or an action outside [0, A).
//   log_probs (nullable): log p_i into log_probs[src_i] for a window, else into log_probs[i]
//   log_mu (nullable [capacity]): with it, rho_i = fminf(rho_bar, expf(log p_i - log_mu[src_i])), NaN where log p_i is
//   NaN or log_mu[src_i] is NaN or > 0; weights_out[i] = (weights_in ? weights_in[i] : 1.0f) * rho_i (weights_out may
//   alias weights_in); rho_out[i] = rho_i (nullable)
struct PolicyLaunch {
    int64_t n, capacity, first;
    const float *states;            // [capacity][12], 16-byte aligned
    const int32_t *actions;         // [capacity]
    const int64_t *idx;             // nullable [n]
    float *log_probs;
    const float *log_mu;
    float rho_bar;
    const float *weights_in;
    float *weights_out, *rho_out;
};
hipError_t launch_learner_policy(const LearnerDevice &d, const PolicyLaunch &q, hipStream_t stream);

}  // namespace uavtrack

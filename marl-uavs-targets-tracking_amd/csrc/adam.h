// adam.h -- what both device trainers keep and step the same way.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace uavtrack {

// What both device trainers (uavtrack_learner_*, uavtrack_pmi_trainer_*) keep the same way: the torch.optim.Adam state
// of their trainable tensors and the words through which a call is refused on the device.  api_handle.h owns its buffers
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

}  // namespace uavtrack

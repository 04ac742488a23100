// api_env.h -- the two bridges from the device trainers into the environment handle (api_env.hip).
#pragma once

#include "api_common.h"
#include "env.h"

namespace uavtrack {

// the device pack behind uavtrack_publish_actor_weights and uavtrack_learner_publish_actor
int publish_actor(const char *fn, uavtrack_env *env, const float *w1, const float *b1, const float *w2, const float *b2,
                  int32_t hidden, int32_t n_actions, void *stream);
// the device pack behind uavtrack_publish_pmi_weights and uavtrack_pmi_trainer_publish
int publish_pmi(const char *fn, uavtrack_env *env, const float *const tensors[kPmiStateTensors], int32_t hidden,
                void *stream);

}  // namespace uavtrack

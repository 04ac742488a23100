// lds.h -- the LDS of a gfx950 compute unit, as the rollout (env.h) and the episode results (episode.h) size against it.
#pragma once

#include <stddef.h>

namespace uavtrack {

constexpr size_t kLdsSoft = 64 * 1024;    // dynamic LDS a launch gets without asking
constexpr size_t kLdsMax = 160 * 1024;    // LDS of a gfx950 CU: what one workgroup may take (hipFuncAttributeMaxDynamicSharedMemorySize)

}  // namespace uavtrack

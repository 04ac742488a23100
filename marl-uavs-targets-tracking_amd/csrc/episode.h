// episode.h -- per-episode results (uavtrack_episode_stats_*): what episode_kernel.hip and api_episode.hip share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lds.h"
#include "uavtrack.h"

namespace uavtrack {

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

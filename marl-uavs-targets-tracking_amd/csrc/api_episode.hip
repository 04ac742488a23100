// api_episode.hip -- the C ABI of the per-episode results (include/uavtrack.h, uavtrack_episode_stats_*).

#include "api_handle.h"
#include "episode.h"

using namespace uavtrack;

struct uavtrack_episode_stats {
    uavtrack_episode_stats_config cfg;
    EpisodeDevice d;
};

namespace uavtrack {

static Bufs device_bufs(EpisodeDevice &d)
{
    const size_t B = (size_t)d.B;
    return {buf(d.step_sums, (size_t)d.max_steps * 4 * B), buf(d.acc, 4 * B, true), buf(d.cov_sum, B, true),
            buf(d.cov_max, B, true), buf(d.steps, B, true), buf(d.ordinal, B, true),
            buf(d.slots, (size_t)d.max_steps * (size_t)episode_groups(d.B)), buf(d.head, 3, true),
            buf(d.log, (size_t)d.log_capacity)};
}

}  // namespace uavtrack

extern "C" {

int uavtrack_episode_stats_create(const uavtrack_episode_stats_config *cfg, uavtrack_episode_stats **out)
{
    auto check = [](const char *fn, const uavtrack_episode_stats_config &c) {
        if (c.n_envs < 1) return fail("%s: n_envs %lld < 1", fn, (long long)c.n_envs);
        if (c.n_uav < 1 || c.n_uav > kEpisodeMaxUav) return fail("%s: n_uav %d out of range [1, %d]", fn, c.n_uav, kEpisodeMaxUav);
        if (c.max_steps < 1) return fail("%s: max_steps %lld < 1", fn, (long long)c.max_steps);
        if (c.max_steps > INT32_MAX / c.n_envs)
            return fail("%s: max_steps %lld * n_envs %lld must stay below 2^31", fn, (long long)c.max_steps, (long long)c.n_envs);
        if (c.log_capacity < 1 || c.log_capacity > INT32_MAX)
            return fail("%s: log_capacity %lld out of range [1, 2^31)", fn, (long long)c.log_capacity);
        return 0;
    };
    auto init = [](EpisodeDevice &d, const uavtrack_episode_stats_config &c) {
        d.B = c.n_envs;
        d.N = c.n_uav;
        d.env_offset = c.env_offset;
        d.max_steps = c.max_steps;
        d.log_capacity = c.log_capacity;
        return hipSuccess;
    };
    return create_handle(__func__, cfg, out, check, init);
}

int uavtrack_episode_stats_destroy(uavtrack_episode_stats *stats) { return destroy_handle(stats); }

int uavtrack_episode_stats_add(uavtrack_episode_stats *stats, int64_t T, const float *reward, const float *terms,
                               const int32_t *covered, const uint8_t *done, void *stream)
{
    if (!stats) return fail("uavtrack_episode_stats_add: null handle");
    if (!reward || !terms || !covered) return fail("uavtrack_episode_stats_add: reward, terms and covered must not be null");
    if (T < 1 || T > stats->cfg.max_steps)
        return fail("uavtrack_episode_stats_add: T = %lld outside [1, max_steps = %lld]", (long long)T,
                    (long long)stats->cfg.max_steps);
    ON_DEVICE(stats->cfg.device_id);
    HIP_TRY(launch_episode_add(stats->d, T, reward, terms, covered, done, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_episode_stats_close(uavtrack_episode_stats *stats, void *stream)
{
    if (!stats) return fail("uavtrack_episode_stats_close: null handle");
    ON_DEVICE(stats->cfg.device_id);
    HIP_TRY(launch_episode_close(stats->d, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_episode_stats_read(uavtrack_episode_stats *stats, uavtrack_episode_record *records_host, int64_t capacity,
                                int64_t *count, int64_t *dropped, void *stream)
{
    if (!stats || !count || !dropped) return fail("uavtrack_episode_stats_read: null argument");
    if (capacity < 0 || (capacity > 0 && !records_host))
        return fail("uavtrack_episode_stats_read: capacity %lld without a record array", (long long)capacity);
    ON_DEVICE(stats->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    int64_t head[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(head, stats->d.head, sizeof head, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n = head[0] < capacity ? head[0] : capacity;
    if (n > 0) {
        HIP_TRY(hipMemcpyAsync(records_host, stats->d.log, (size_t)n * sizeof(uavtrack_episode_record), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    *count = head[0];
    *dropped = head[1];
    return 0;
}

int uavtrack_episode_stats_clear(uavtrack_episode_stats *stats, void *stream)
{
    if (!stats) return fail("uavtrack_episode_stats_clear: null handle");
    ON_DEVICE(stats->cfg.device_id);
    HIP_TRY(hipMemsetAsync(stats->d.head, 0, 2 * sizeof(int64_t), static_cast<hipStream_t>(stream)));
    return 0;
}

}  // extern "C"

/* The refusals of the five ring adds (uavtrack_replay_add*), driven on the host alone: api_replay.hip is compiled into
 * this program, the handle is a plain struct that no device ever saw, and every call below is refused before anything
 * reaches the HIP runtime.  It is the fault table of tests/test_hip_replay_add_forms.py without the cases that need a
 * live handle (the good call, the ring image), and exists so the acceptor can run under the host sanitizers:
 *
 *   hipcc --offload-arch=gfx950 -std=c++17 -Iinclude -Imarl-uavs-targets-tracking_amd/csrc \
 *         -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer \
 *         tests/abi/replay_add_refusals.hip -o replay_add_refusals \
 *         -Lmarl-uavs-targets-tracking_amd/uavtrack -luavtrack -Wl,-rpath,$PWD/marl-uavs-targets-tracking_amd/uavtrack
 *
 * (the library supplies the error string and the launchers the accepted path would call).  Exit status 0 and
 * "N refusals, 0 wrong". */
#include "api_replay.hip"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

constexpr int64_t kCap = 100, kT = 3, kB = 2, kN = 7;
alignas(16) float rows[64];             // stands for every device array: the acceptor looks at addresses only
int checked = 0, wrong = 0;

struct Args {
    uavtrack_replay *h;
    const uavtrack_replay_ring *ring;
    float *discounts = rows;
    int64_t steps = kT, envs = kB, n_uav = kN;
    const float *obs_in = rows, *obs = rows, *reward = rows, *start_obs = rows, *values = rows;
    const int32_t *actions = reinterpret_cast<const int32_t *>(rows);
    const uint8_t *done = reinterpret_cast<const uint8_t *>(rows);
    int32_t n_step = 3;
    double lambda = 0.9, gamma = 0.95;
};

// form 0..4: add, add_rollout, _episodes, _nstep, _lambda (the flat form takes obs_in / obs as states / next_states)
const char *const kNames[5] = {"uavtrack_replay_add", "uavtrack_replay_add_rollout", "uavtrack_replay_add_rollout_episodes",
                               "uavtrack_replay_add_rollout_nstep", "uavtrack_replay_add_rollout_lambda"};

int call(int form, const Args &a)
{
    switch (form) {
    case 0: return uavtrack_replay_add(a.h, a.ring, a.steps, a.obs_in, a.actions, a.reward, a.obs, nullptr);
    case 1: return uavtrack_replay_add_rollout(a.h, a.ring, a.steps, a.envs, a.obs_in, a.obs, a.actions, a.reward, nullptr);
    case 2: return uavtrack_replay_add_rollout_episodes(a.h, a.ring, a.steps, a.envs, a.n_uav, a.obs_in, a.obs, a.actions,
                                                        a.reward, a.done, a.start_obs, nullptr);
    case 3: return uavtrack_replay_add_rollout_nstep(a.h, a.ring, a.discounts, a.steps, a.envs, a.n_uav, a.obs_in, a.obs,
                                                     a.actions, a.reward, a.done, a.start_obs, a.n_step, a.gamma, nullptr);
    default: return uavtrack_replay_add_rollout_lambda(a.h, a.ring, a.discounts, a.steps, a.envs, a.n_uav, a.obs_in, a.obs,
                                                       a.actions, a.reward, a.done, a.start_obs, a.values, a.lambda, a.gamma,
                                                       nullptr);
    }
}

void refused(int form, const char *label, const Args &a, const std::string &text)
{
    const int rc = call(form, a);
    const std::string want = std::string(kNames[form]) + ": " + text;
    ++checked;
    if (rc != 0 && want == uavtrack_last_error()) return;
    ++wrong;
    std::fprintf(stderr, "%s, %s: rc %d\n  got  %s\n  want %s\n", kNames[form], label, rc, uavtrack_last_error(), want.c_str());
}

}  // namespace

int main()
{
    uavtrack_replay handle{};
    handle.cfg.max_capacity = kCap;
    handle.cfg.max_batch = 16;
    uavtrack_replay_ring good{};
    good.states = good.rewards = good.next_states = rows;
    good.actions = reinterpret_cast<int32_t *>(rows);
    good.capacity = kCap; good.pos = 97; good.count = 97;
    const float *off = rows + 1;                // 4 bytes off a 16-byte boundary
    const char *null_names[5] = {"states, actions, rewards and next_states", "obs_in, obs, actions and reward",
                                 "obs_in, obs, actions, reward, done and start_obs",
                                 "discounts, obs_in, obs, actions and reward",
                                 "discounts, obs_in, obs, actions, reward and values"};
    const char *aligned_names[5] = {"states and next_states", "obs_in and obs", "obs_in, obs and start_obs",
                                    "obs_in, obs and start_obs", "obs_in, obs and start_obs"};
    for (int form = 0; form < 5; ++form) {
        Args base;
        base.h = &handle; base.ring = &good;
        Args a = base;
        a.h = nullptr;
        refused(form, "null handle", a, "null handle");
        a = base; a.ring = nullptr;
        refused(form, "null ring", a, "ring is null");

        uavtrack_replay_ring r = good;
        a = base; a.ring = &r;
        r.pos = kCap;
        refused(form, "pos == capacity", a, "pos 100 outside [0, capacity = 100)");
        r = good; r.capacity = kCap + 1;
        refused(form, "capacity > max_capacity", a, "capacity 101 outside [1, max_capacity = 100]");
        r = good; r.count = kCap + 1;
        refused(form, "count > capacity", a, "count 101 outside [0, capacity = 100]");
        const std::string stores = "the ring's states, actions, rewards and next_states must not be null";
        r = good; r.states = nullptr;      refused(form, "ring.states null", a, stores);
        r = good; r.actions = nullptr;     refused(form, "ring.actions null", a, stores);
        r = good; r.rewards = nullptr;     refused(form, "ring.rewards null", a, stores);
        r = good; r.next_states = nullptr; refused(form, "ring.next_states null", a, stores);
        const std::string store_align = "the ring's states and next_states must be 16-byte aligned";
        r = good; r.states = rows + 1;      refused(form, "ring.states + 4", a, store_align);
        r = good; r.next_states = rows + 1; refused(form, "ring.next_states + 4", a, store_align);

        const std::string nulls = std::string(null_names[form]) + " must not be null";
        a = base; a.obs_in = nullptr;  refused(form, "obs_in / states null", a, nulls);
        a = base; a.obs = nullptr;     refused(form, "obs / next_states null", a, nulls);
        a = base; a.actions = nullptr; refused(form, "actions null", a, nulls);
        a = base; a.reward = nullptr;  refused(form, "reward null", a, nulls);
        if (form == 2) {
            a = base; a.done = nullptr;      refused(form, "done null", a, nulls);
            a = base; a.start_obs = nullptr; refused(form, "start_obs null", a, nulls);
        }
        if (form >= 3) { a = base; a.discounts = nullptr; refused(form, "discounts null", a, nulls); }
        if (form == 4) { a = base; a.values = nullptr; refused(form, "values null", a, nulls); }
        if (form >= 3) {
            const std::string pair = "done and start_obs must both be given or both be null";
            a = base; a.done = nullptr;      refused(form, "only done null", a, pair);
            a = base; a.start_obs = nullptr; refused(form, "only start_obs null", a, pair);
        }
        const std::string aligns = std::string(aligned_names[form]) + " must be 16-byte aligned";
        a = base; a.obs_in = off; refused(form, "obs_in / states + 4", a, aligns);
        a = base; a.obs = off;    refused(form, "obs / next_states + 4", a, aligns);
        if (form >= 2) { a = base; a.start_obs = off; refused(form, "start_obs + 4", a, aligns); }

        if (form == 3)
            for (int v : {0, 65}) {
                a = base; a.n_step = v;
                refused(form, "n_step", a, "n_step = " + std::to_string(v) + " outside [1, 64]");
            }
        const double bad[4] = {NAN, -0.1, 1.5, INFINITY};
        const char *bad_text[4] = {"nan", "-0.1", "1.5", "inf"};
        for (int k = 0; k < 4 && form >= 3; ++k) {
            if (form == 4) {
                a = base; a.lambda = bad[k];
                refused(form, "lambda", a, std::string("lambda = ") + bad_text[k] + " is not a finite value in [0, 1]");
            }
            a = base; a.gamma = bad[k];
            refused(form, "gamma", a, std::string("gamma = ") + bad_text[k] + " is not a finite value in [0, 1]");
        }

        if (form == 0) {
            a = base; a.steps = 0; refused(form, "n = 0", a, "n = 0 < 1");
            continue;
        }
        const std::string sizes = form == 1 ? "steps and agents must be >= 1" : "steps, envs and n_uav must be >= 1";
        const std::string over = form == 1 ? "steps * agents overflows" : "steps * envs * n_uav overflows";
        a = base; a.steps = 0; refused(form, "steps = 0", a, sizes);
        a = base; a.envs = 0;  refused(form, "envs / agents = 0", a, sizes);
        a = base; a.steps = (int64_t)1 << 62; refused(form, "steps = 2^62", a, over);
        if (form >= 2) {
            a = base; a.n_uav = 0; refused(form, "n_uav = 0", a, sizes);
            a = base; a.envs = (int64_t)1 << 62; refused(form, "envs = 2^62", a, over);
        }
    }
    std::printf("%d refusals, %d wrong\n", checked, wrong);
    return wrong ? 1 : 0;
}

// api_pmi_trainer.hip -- the C ABI of the device PMI trainer (include/uavtrack.h, uavtrack_pmi_trainer_*).

#include "api_env.h"
#include "api_handle.h"
#include "pmi_train.h"

#include <cmath>

using namespace uavtrack;

struct uavtrack_pmi_trainer {
    uavtrack_pmi_trainer_config cfg;
    PmiTrainDevice d;
};

namespace uavtrack {

static Bufs scratch_bufs(PmiTrainDevice &d, int64_t max_b)
{
    const size_t H = (size_t)d.L.H, nb = (size_t)max_b;
    return {buf(d.xh0, 2 * 3 * H * nb), buf(d.a0, 2 * 3 * H * nb), buf(d.da0, 2 * 3 * H * nb), buf(d.xh1, 2 * H * nb),
            buf(d.a1, 2 * H * nb), buf(d.dz1, 2 * H * nb), buf(d.go, 2 * nb), buf(d.sel, 2 * 12 * nb), buf(d.sel_t, nb),
            buf(d.sel_u, 2 * nb)};
}

static Bufs device_bufs(PmiTrainDevice &d)
{
    const size_t S = (size_t)d.L.S, P = (size_t)d.L.P, H = (size_t)d.L.H;
    return adam_bufs(d.opt) + Bufs{buf(d.state, S, true), buf(d.nbt, kPmiBlocks, true), buf(d.grad, P, true),
                                   buf(d.inv0, 2 * 3 * H), buf(d.inv1, 2 * H), buf(d.acc, 1)} +
           scratch_bufs(d, d.max_b);
}

static int *refusal_word(const PmiTrainDevice &d) { return d.opt.errors; }

}  // namespace uavtrack

namespace {

constexpr int64_t kPmiTrainDefaultBatch = 4096;

// The batch tests of uavtrack_pmi_trainer_train and _train_many: batch_size, the reserved scratch, and b2 against it.
int accept_pmi_batch(const char *fn, const uavtrack_pmi_trainer *trainer, int64_t batch_size, int64_t b2)
{
    if (batch_size < 2)
        return fail("%s: batch_size = %lld < 2 (train-mode BatchNorm1d needs two rows)", fn, (long long)batch_size);
    if (batch_size > trainer->d.max_b)
        return fail("%s: batch_size = %lld, scratch is reserved for %lld (uavtrack_pmi_trainer_reserve)", fn,
                    (long long)batch_size, (long long)trainer->d.max_b);
    if (b2 < batch_size)
        return fail("%s: b2 = %lld < batch_size = %lld (no mini-batch)", fn, (long long)b2, (long long)batch_size);
    if (b2 / batch_size > (int64_t)1 << 30) return fail("%s: b2 = %lld too large", fn, (long long)b2);
    return 0;
}

// The source list of uavtrack_pmi_trainer_train_many / _select into the table the select kernel takes by value; the
// span starts at group_base.  Returns nonzero after fail().
int accept_sources(const char *fn, const uavtrack_pmi_source *sources, int32_t count, int64_t n_uav, int64_t group_base,
                   PmiSourceTable *out)
{
    if (!sources) return fail("%s: sources must not be null", fn);
    if (count < 1 || count > UAVTRACK_PMI_MAX_SOURCES)
        return fail("%s: count = %d out of range [1, %d]", fn, count, UAVTRACK_PMI_MAX_SOURCES);
    if (n_uav < 1) return fail("%s: n_uav = %lld < 1", fn, (long long)n_uav);
    out->count = count;
    out->base[0] = group_base;
    for (int k = 0; k < count; ++k) {
        if (!sources[k].rows) return fail("%s: sources[%d].rows is null", fn, k);
        if (sources[k].n_rows < n_uav || sources[k].n_rows % n_uav != 0)
            return fail("%s: sources[%d].n_rows = %lld is not a positive multiple of n_uav = %lld", fn, k,
                        (long long)sources[k].n_rows, (long long)n_uav);
        const int64_t groups = sources[k].n_rows / n_uav;
        if (groups > INT64_MAX / 2 - out->base[k]) return fail("%s: the sources hold too many groups", fn);
        out->rows[k] = sources[k].rows;
        out->base[k + 1] = out->base[k] + groups;
    }
    for (int k = count; k < kPmiMaxSources; ++k) {
        out->rows[k] = nullptr;
        out->base[k + 1] = out->base[count];
    }
    return 0;
}

}  // namespace

extern "C" {

int uavtrack_pmi_trainer_create(const uavtrack_pmi_trainer_config *cfg, uavtrack_pmi_trainer **out)
{
    auto check = [](const char *fn, const uavtrack_pmi_trainer_config &c) {
        if (c.hidden < 1 || c.hidden > kPmiMaxHidden)
            return fail("%s: hidden %d out of range [1, %d]", fn, c.hidden, kPmiMaxHidden);
        if (c.max_batch < 0 || c.max_batch > kPmiTrainMaxBatch)
            return fail("%s: max_batch %lld out of range [0, %lld]", fn, (long long)c.max_batch, (long long)kPmiTrainMaxBatch);
        if (!std::isfinite(c.lr) || c.lr < 0) return fail("%s: lr must be finite and >= 0", fn);
        return 0;
    };
    auto init = [](PmiTrainDevice &d, const uavtrack_pmi_trainer_config &c) {
        d.L = PmiTrainLayout::make(c.hidden);
        d.lr = (float)c.lr;
        d.opt.tensors = kPmiTrainTensors;
        d.opt.P = d.L.P;
        d.max_b = c.max_batch ? c.max_batch : kPmiTrainDefaultBatch;
        return hipSuccess;
    };
    return create_handle(__func__, cfg, out, check, init);
}

int uavtrack_pmi_trainer_destroy(uavtrack_pmi_trainer *trainer) { return destroy_handle(trainer); }

int uavtrack_pmi_trainer_num_params(uavtrack_pmi_trainer *trainer, int64_t *n_state, int64_t *n_train)
{
    if (!trainer || !n_state || !n_train) return fail("uavtrack_pmi_trainer_num_params: null argument");
    *n_state = trainer->d.L.S;
    *n_train = trainer->d.L.P;
    return 0;
}

int uavtrack_pmi_trainer_reserve(uavtrack_pmi_trainer *trainer, int64_t max_batch)
{
    return reserve_scratch(__func__, trainer, max_batch, kPmiTrainMaxBatch, &PmiTrainDevice::max_b);
}

int uavtrack_pmi_trainer_set_params(uavtrack_pmi_trainer *trainer, const float *state, const int64_t *num_batches_tracked,
                                    int64_t n_state, void *stream)
{
    if (!trainer || !state || !num_batches_tracked) return fail("uavtrack_pmi_trainer_set_params: null argument");
    PmiTrainDevice &d = trainer->d;
    if (n_state != d.L.S)
        return fail("uavtrack_pmi_trainer_set_params: %lld floats, the network's state has %d", (long long)n_state, d.L.S);
    for (int b = 0; b < kPmiBlocks; ++b)
        if (num_batches_tracked[b] < 0)
            return fail("uavtrack_pmi_trainer_set_params: num_batches_tracked[%d] = %lld < 0", b,
                        (long long)num_batches_tracked[b]);
    ON_DEVICE(trainer->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpyAsync(d.state, state, (size_t)n_state * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d.nbt, num_batches_tracked, kPmiBlocks * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int uavtrack_pmi_trainer_get_params(uavtrack_pmi_trainer *trainer, float *state, int64_t *num_batches_tracked,
                                    int64_t n_state, void *stream)
{
    if (!trainer || !state || !num_batches_tracked) return fail("uavtrack_pmi_trainer_get_params: null argument");
    PmiTrainDevice &d = trainer->d;
    if (n_state != d.L.S)
        return fail("uavtrack_pmi_trainer_get_params: %lld floats, the network's state has %d", (long long)n_state, d.L.S);
    ON_DEVICE(trainer->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(state, d.state, (size_t)n_state * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(num_batches_tracked, d.nbt, kPmiBlocks * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int uavtrack_pmi_trainer_publish(uavtrack_pmi_trainer *trainer, uavtrack_env *env, void *stream)
{
    if (!trainer || !env) return fail("uavtrack_pmi_trainer_publish: null handle");
    if (trainer->cfg.device_id != env->cfg.device_id)
        return fail("uavtrack_pmi_trainer_publish: the trainer is on device %d, the environment on device %d",
                    trainer->cfg.device_id, env->cfg.device_id);
    const PmiTrainLayout &L = trainer->d.L;
    const float *p[kPmiStateTensors];
    for (int k = 0; k < kPmiStateTensors; ++k) p[k] = trainer->d.state + L.soff[k];
    return publish_pmi(__func__, env, p, L.H, stream);
}

int uavtrack_pmi_trainer_set_optimizer_state(uavtrack_pmi_trainer *trainer, const float *exp_avg, const float *exp_avg_sq,
                                             const int64_t *step, int64_t n_train, void *stream)
{
    return optimizer_state(__func__, trainer, exp_avg, exp_avg_sq, step, n_train, stream, "the network has %d trainable");
}

int uavtrack_pmi_trainer_get_optimizer_state(uavtrack_pmi_trainer *trainer, float *exp_avg, float *exp_avg_sq,
                                             int64_t *step, int64_t n_train, void *stream)
{
    return optimizer_state(__func__, trainer, exp_avg, exp_avg_sq, step, n_train, stream, "the network has %d trainable");
}

int uavtrack_pmi_trainer_train(uavtrack_pmi_trainer *trainer, const float *rows, int64_t n_rows, int64_t n_uav,
                               const int64_t *t_idx, const int64_t *u_idx, int64_t b2, int64_t batch_size,
                               float *avg_loss, float *losses, float *outputs, void *stream)
{
    if (!trainer) return fail("uavtrack_pmi_trainer_train: null handle");
    if (!rows || !t_idx || !u_idx || !avg_loss)
        return fail("uavtrack_pmi_trainer_train: rows, t_idx, u_idx and avg_loss must not be null");
    if (n_uav < 1) return fail("uavtrack_pmi_trainer_train: n_uav = %lld < 1", (long long)n_uav);
    if (n_rows < n_uav || n_rows % n_uav != 0)
        return fail("uavtrack_pmi_trainer_train: n_rows = %lld is not a positive multiple of n_uav = %lld", (long long)n_rows,
                    (long long)n_uav);
    if (accept_pmi_batch(__func__, trainer, batch_size, b2)) return 1;
    ON_DEVICE(trainer->cfg.device_id);
    PmiTrainLaunch q;
    q.rows = rows; q.n_rows = n_rows; q.n_uav = n_uav; q.b2 = b2; q.batch = batch_size;
    q.t_idx = t_idx; q.u_idx = u_idx; q.avg_loss = avg_loss; q.losses = losses; q.outputs = outputs;
    HIP_TRY(launch_pmi_train(trainer->d, q, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_pmi_trainer_train_many(uavtrack_pmi_trainer *trainer, const uavtrack_pmi_source *sources, int32_t count,
                                    int64_t n_uav, const int64_t *t_idx, const int64_t *u_idx, int64_t b2,
                                    int64_t batch_size, float *avg_loss, float *losses, float *outputs, void *stream)
{
    if (!trainer) return fail("uavtrack_pmi_trainer_train_many: null handle");
    if (!t_idx || !u_idx || !avg_loss)
        return fail("uavtrack_pmi_trainer_train_many: t_idx, u_idx and avg_loss must not be null");
    PmiSourceTable table;
    if (accept_sources(__func__, sources, count, n_uav, 0, &table)) return 1;
    if (accept_pmi_batch(__func__, trainer, batch_size, b2)) return 1;
    ON_DEVICE(trainer->cfg.device_id);
    PmiTrainLaunch q;
    q.rows = nullptr; q.n_rows = table.base[count] * n_uav; q.n_uav = n_uav; q.b2 = b2; q.batch = batch_size;
    q.t_idx = t_idx; q.u_idx = u_idx; q.avg_loss = avg_loss; q.losses = losses; q.outputs = outputs;
    HIP_TRY(launch_pmi_train_many(trainer->d, table, q, static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_pmi_trainer_select(uavtrack_pmi_trainer *trainer, const uavtrack_pmi_source *sources, int32_t count,
                                int64_t group_base, int64_t total_groups, int64_t n_uav, const int64_t *t_idx,
                                const int64_t *u_idx, int64_t b2, float *selected, void *stream)
{
    if (!trainer) return fail("uavtrack_pmi_trainer_select: null handle");
    if (!t_idx || !u_idx || !selected)
        return fail("uavtrack_pmi_trainer_select: t_idx, u_idx and selected must not be null");
    if (b2 < 1 || b2 > INT32_MAX)   // 24 lanes per draw at most: the grid stays below 2^31 workgroups
        return fail("uavtrack_pmi_trainer_select: b2 = %lld out of range [1, %d]", (long long)b2, INT32_MAX);
    if (group_base < 0 || total_groups < 1 || group_base >= total_groups)
        return fail("uavtrack_pmi_trainer_select: group_base = %lld outside a timeline of %lld groups", (long long)group_base,
                    (long long)total_groups);
    PmiSourceTable table;
    if (accept_sources(__func__, sources, count, n_uav, group_base, &table)) return 1;
    if (table.base[count] > total_groups)
        return fail("uavtrack_pmi_trainer_select: the sources end at group %lld of a timeline of %lld", (long long)table.base[count],
                    (long long)total_groups);
    ON_DEVICE(trainer->cfg.device_id);
    HIP_TRY(launch_pmi_select(trainer->d, table, total_groups, n_uav, t_idx, u_idx, b2, selected,
                              static_cast<hipStream_t>(stream)));
    return 0;
}

int uavtrack_pmi_trainer_check(uavtrack_pmi_trainer *trainer, int64_t *refused, void *stream)
{
    int count = 0;
    if (take_refusals(__func__, trainer, refused, stream, &count)) return 1;
    if (count)
        return fail("uavtrack_pmi_trainer_check: %d train call(s) refused: a timestep index outside [0, T) or a uav index "
                    "outside [0, n_uav); they changed nothing", count);
    return 0;
}

}  // extern "C"

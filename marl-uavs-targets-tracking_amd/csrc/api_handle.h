// api_handle.h -- what the four device-side handles (learner, PMI trainer, replay ring, episode results) share: their
// lifetime, their scratch, the trainers' Adam state and the refusal count.  A handle H is {cfg, d}; its translation unit
// states, in namespace uavtrack where the templates below find them by their argument, device_bufs(d) (every device
// buffer, sized from d's fields), scratch_bufs(d, rows) where it has a *_reserve, and refusal_word(d) where it has a
// *_check: the word through which its calls are refused on the device.
#pragma once

#include "adam.h"
#include "api_common.h"

#include <cstdio>
#include <new>
#include <type_traits>

namespace uavtrack {

// The two trainers share the torch.optim.Adam state (AdamState, adam.h).
inline Bufs adam_bufs(AdamState &o)
{
    return {buf(o.m, o.P, true), buf(o.v, o.P, true), buf(o.steps, o.tensors, true), buf(o.status, 1, true),
            buf(o.errors, 1, true)};
}

namespace {      // (file-local in each api_*.hip, as every instantiation is)

// *_create: the null and struct_size tests, the config's ranges (`check`), the device, then the handle with the fields
// `init` derives from the config (it may return an error of its own), every buffer of device_bufs() at once, and a
// device synchronisation.  A failure leaves nothing behind.
template <typename H, typename Cfg, typename Check, typename Init>
int create_handle(const char *fn, const Cfg *cfg, H **out, Check check, Init init)
{
    if (!cfg || !out) return fail("%s: null argument", fn);
    *out = nullptr;
    if (cfg->struct_size != sizeof(Cfg))
        return fail("%s: struct_size %u != %zu (header / library mismatch)", fn, cfg->struct_size, sizeof(Cfg));
    if (check(fn, *cfg)) return 1;
    hipDeviceProp_t prop;
    if (accept_device(fn, cfg->device_id, &prop)) return 1;
    ON_DEVICE(cfg->device_id);
    H *h = new (std::nothrow) H();
    if (!h) return fail("%s: out of host memory", fn);
    h->cfg = *cfg;
    hipError_t e = init(h->d, *cfg);
    if (e == hipSuccess) e = replace(device_bufs(h->d));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        release(device_bufs(h->d));
        delete h;
        return fail("%s: %s", fn, hipGetErrorString(e));
    }
    *out = h;
    return 0;
}

template <typename H>
int destroy_handle(H *h)
{
    if (!h) return 0;
    DeviceGuard guard(h->cfg.device_id);
    (void)hipDeviceSynchronize();
    release(device_bufs(h->d));
    delete h;
    return 0;
}

// *_reserve: scratch for `max_batch` rows (grow-only; `rows` holds what is reserved), the new set allocated before the
// old one goes.
template <typename H, typename D>
int reserve_scratch(const char *fn, H *h, int64_t max_batch, int64_t limit, int64_t D::*rows)
{
    if (!h) return fail("%s: null handle", fn);
    if (max_batch < 1 || max_batch > limit)
        return fail("%s: max_batch %lld out of range [1, %lld]", fn, (long long)max_batch, (long long)limit);
    if (max_batch <= h->d.*rows) return 0;
    ON_DEVICE(h->cfg.device_id);
    HIP_TRY(hipDeviceSynchronize());          // in-flight calls may still use the old scratch
    HIP_TRY(replace(scratch_bufs(h->d, max_batch)));
    h->d.*rows = max_batch;
    return 0;
}

// *_set/get_optimizer_state of a trainer: exp_avg, exp_avg_sq [P] and step [tensors] in from the host (const
// pointers; everything is validated before the first copy, so a refused load leaves the previous state in place) or
// out to it.  `has` completes the size message: "<n> floats, <has % P>".
template <typename H, typename F, typename S>
int optimizer_state(const char *fn, H *h, F *exp_avg, F *exp_avg_sq, S *step, int64_t n_floats, void *stream,
                    const char *has)
{
    if (!h || !exp_avg || !exp_avg_sq || !step) return fail("%s: null argument", fn);
    const AdamState &o = h->d.opt;
    if (n_floats != h->d.L.P) {
        char what[96];
        snprintf(what, sizeof what, has, h->d.L.P);
        return fail("%s: %lld floats, %s", fn, (long long)n_floats, what);
    }
    ON_DEVICE(h->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if constexpr (std::is_const<F>::value) {
        for (int t = 0; t < o.tensors; ++t)
            if (step[t] < 0) return fail("%s: step[%d] = %lld < 0", fn, t, (long long)step[t]);
        for (int64_t p = 0; p < o.P; ++p)
            if (!(exp_avg_sq[p] >= 0.0f)) return fail("%s: exp_avg_sq[%lld] is not >= 0", fn, (long long)p);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpyAsync(o.m, exp_avg, (size_t)o.P * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.v, exp_avg_sq, (size_t)o.P * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(o.steps, step, (size_t)o.tensors * 8, hipMemcpyHostToDevice, st));
    } else {
        HIP_TRY(hipMemcpyAsync(exp_avg, o.m, (size_t)o.P * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(exp_avg_sq, o.v, (size_t)o.P * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(step, o.steps, (size_t)o.tensors * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// *_check: the calls refused on the device since the last check (`count`, and `refused` when given), the count
// cleared; synchronises the stream.
template <typename H>
int take_refusals(const char *fn, H *h, int64_t *refused, void *stream, int *count)
{
    if (!h) return fail("%s: null handle", fn);
    ON_DEVICE(h->cfg.device_id);
    hipStream_t st = static_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(count, refusal_word(h->d), 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(refusal_word(h->d), 0, 4, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (refused) *refused = *count;
    return 0;
}

}  // namespace

}  // namespace uavtrack

// api_common.hip -- the one error string of libuavtrack.so and the helpers every api_*.hip shares (api_common.h).

#include "api_common.h"
#include "uavtrack.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>

namespace {

thread_local std::string g_err;

}  // namespace

namespace uavtrack {

int fail(const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

void release(const Bufs &set)
{
    for (const Buf &b : set) {
        if (*b.slot) (void)hipFree(*b.slot);
        *b.slot = nullptr;
    }
}

hipError_t replace(const Bufs &set, hipStream_t st)
{
    std::vector<void *> fresh(set.size(), nullptr);
    hipError_t e = hipSuccess;
    for (size_t i = 0; i < set.size() && e == hipSuccess; ++i) e = hipMalloc(&fresh[i], set[i].bytes);
    for (size_t i = 0; i < set.size() && e == hipSuccess; ++i)
        if (set[i].zero) e = hipMemsetAsync(fresh[i], 0, set[i].bytes, st);
    if (e != hipSuccess) {
        for (void *p : fresh)
            if (p) (void)hipFree(p);
        return e;
    }
    release(set);
    for (size_t i = 0; i < set.size(); ++i) *set[i].slot = fresh[i];
    return hipSuccess;
}

int accept_device(const char *fn, int device_id, hipDeviceProp_t *prop)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1)
        return fail("%s: no HIP device visible (%s); libuavtrack has no CPU fallback", fn,
                    e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (device_id < 0 || device_id >= ndev) return fail("%s: device_id %d out of range [0, %d)", fn, device_id, ndev);
    HIP_TRY(hipGetDeviceProperties(prop, device_id));
    if (strncmp(prop->gcnArchName, "gfx950", 6) != 0)
        return fail("%s: device %d is %s; this library is built for gfx950 only", fn, device_id, prop->gcnArchName);
    return 0;
}

}  // namespace uavtrack

extern "C" {

int uavtrack_version(void) { return UAVTRACK_ABI_VERSION; }

const char *uavtrack_last_error(void) { return g_err.c_str(); }

}  // extern "C"

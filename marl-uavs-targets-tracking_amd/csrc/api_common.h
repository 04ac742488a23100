// api_common.h -- what every translation unit of the C ABI (api_*.hip) uses: the error string, the device guard and the
// lists of device buffers.  The definitions are in api_common.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>

#include <vector>

namespace uavtrack {

// sets the thread's error string (uavtrack_last_error); returns 1
int fail(const char *fmt, ...);

#define HIP_TRY(expr)                                                                  \
    do {                                                                               \
        hipError_t e__ = (expr);                                                       \
        if (e__ != hipSuccess) return fail("%s: %s", #expr, hipGetErrorString(e__));   \
    } while (0)

// Makes the handle's device current for the duration of one ABI call and gives the caller's device back on
// return: a process that drives several shards, or keeps PyTorch on another GPU, must not find its current
// device changed behind its back.
namespace {
struct DeviceGuard {
    int prev = -1;
    bool changed = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev)
    {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            changed = (err == hipSuccess);
        }
    }
    ~DeviceGuard()
    {
        if (changed) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
}  // namespace
#define ON_DEVICE(dev)            \
    DeviceGuard guard__(dev);     \
    HIP_TRY(guard__.err)

// ---- device buffers: each one is named once, in the list of the set it belongs to, for allocation and release alike
struct Buf {
    void **slot;     // the pointer that owns it
    size_t bytes;    // (read by replace() only: release() takes the same lists)
    bool zero;       // starts zeroed
};
using Bufs = std::vector<Buf>;

template <typename T>
Buf buf(T *&p, size_t n = 0, bool zero = false)
{
    return {reinterpret_cast<void **>(&p), (n ? n : 1) * sizeof(T), zero};
}

inline Bufs operator+(Bufs a, const Bufs &b)
{
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

void release(const Bufs &set);

// All or nothing: a new buffer for every slot of `set`, zeroed on `st` where marked, before any slot changes; only then
// are the old buffers freed.  On failure the new ones are freed, every slot keeps what it held, and the error comes back
// (grown scratch: the handle stays good at its old size).
hipError_t replace(const Bufs &set, hipStream_t st = nullptr);

// The device a handle is created on (`fn` names the creating ABI function in the error): visible, and a gfx950.
int accept_device(const char *fn, int device_id, hipDeviceProp_t *prop);

}  // namespace uavtrack

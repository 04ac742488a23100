// episode_kernel.hip -- the reference's per-episode results (train.py:181-196, ReturnValueOfTrain) on the device, from
// the outputs a stepping launch has already written: reward [T][B][N], terms [T][3][B][N], covered [T][B], done [T][B].
//
// One add is a chain of stream-ordered launches, none of which synchronises or allocates:
//   episode_step_sums_kernel  one workgroup per (t, tile of consecutive environments).  For a fixed t the tile's reward
//                             rows and each of its three term planes are contiguous: they are streamed with 16-byte
//                             loads into LDS, then one lane per (plane, environment) adds its N values in ascending
//                             UAV index in fp64 and leaves the step sum in scratch [T][4][B].  The only kernel with
//                             real traffic: 16 bytes per agent-step.
//   episode_count_kernel      (with a done matrix) one wavefront per (t, group of 64 environments): how many of the
//                             group's environments close at t;
//   episode_scan_kernel       one workgroup: those counts -> their exclusive prefix in (t, group) order, i.e. the rank of
//                             every closing step in a scan over the done matrix; the log's fill and its dropped count
//                             advance here, in one thread, from the total;
//   episode_fold_kernel       one workgroup per group, one wavefront per plane, one lane per environment: walks t in
//                             order over the step sums, covered and done; a closing step's record goes to slot
//                             (fill before the call) + prefix[t][group] + (closing lanes below it in the wavefront).
// close is the same chain with "holds at least one step" in place of the done flag.  No atomics anywhere: the log's
// order is the scan's, and every sum has one order (include/uavtrack.h states it).

#include "episode.h"

#include <hip/hip_runtime.h>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kEW = 256;                       // threads per workgroup of the step-sum, count and fold kernels
constexpr int kPlanes = 4;                     // reward, tracking, boundary, duplicate
constexpr int kStageFloats = 3968;             // floats of one plane a tile stages: with the skew below, 4 planes fit 64 KiB
constexpr int kFoldUnroll = 8;                 // steps whose loads the fold issues before it adds the first
constexpr int kScanW = 1024;                   // threads of the scan kernel
static_assert(kEW == kPlanes * kEpisodeGroup, "one wavefront per plane");
static_assert(kStageFloats >= kEpisodeMaxUav, "a tile holds at least one environment");
static_assert(kPlanes * (kStageFloats + (kStageFloats >> 5) + 1) * sizeof(float) <= kLdsSoft, "staging LDS");

// LDS position of a plane's element idx: one dead word behind every 32.  The adding lanes read with a stride of N
// words, which is no power of two in general but shares factors with the 32 banks (N = 20: 4-way); the skew moves
// each 32-word row on by one bank (N = 20, 50, 70: at most 2-way; N = 32: none; N = 64: 2-way).
__device__ __forceinline__ int skew(int idx) { return idx + (idx >> 5); }

__global__ void __launch_bounds__(kEW) episode_step_sums_kernel(const float *reward, const float *terms, double *sums,
                                                                int64_t B, int N, int E, int tiles, int plane_floats)
{
    extern __shared__ __attribute__((aligned(16))) float stage[];
    const int tid = threadIdx.x;
    const int64_t t = blockIdx.x / tiles;
    const int64_t b0 = (int64_t)(blockIdx.x % tiles) * E;
    const int ecur = (int)(B - b0 < E ? B - b0 : E);
    const int n = ecur * N;                    // <= kStageFloats
#pragma unroll
    for (int p = 0; p < kPlanes; ++p) {
        const float *src = p == 0 ? reward + (t * B + b0) * N : terms + ((t * 3 + (p - 1)) * B + b0) * N;
        float *dst = stage + p * plane_floats;
        // scalar words up to the first 16-byte boundary, 16-byte loads, scalar words behind the last one
        const int lead = (int)((4 - (((uintptr_t)src >> 2) & 3)) & 3);
        const int head = lead < n ? lead : n;
        const int nv = (n - head) >> 2;
        const int tail = head + 4 * nv;
        if (tid < head) dst[skew(tid)] = src[tid];
        const float4 *src4 = reinterpret_cast<const float4 *>(src + head);
        for (int v = tid; v < nv; v += kEW) {
            const float4 x = src4[v];
            const int i = head + 4 * v;
            dst[skew(i)] = x.x;
            dst[skew(i + 1)] = x.y;
            dst[skew(i + 2)] = x.z;
            dst[skew(i + 3)] = x.w;
        }
        if (tid < n - tail) dst[skew(tail + tid)] = src[tail + tid];
    }
    __syncthreads();
    const int p = tid >> 6, j = tid & 63;
    if (j < ecur) {
        const float *pl = stage + p * plane_floats;
        double s = 0.0;
        int idx = j * N;
        for (int i = 0; i < N; ++i, ++idx) s += (double)pl[skew(idx)];     // ascending UAV index
        sums[(t * kPlanes + p) * B + b0 + j] = s;
    }
}

// does environment b close at row t?  (add: its done flag; close: it holds at least one step)
__device__ __forceinline__ bool closes(const uint8_t *done, const int32_t *steps, int64_t t, int64_t b, int64_t B)
{
    return done ? done[t * B + b] != 0 : steps[b] > 0;
}

__global__ void __launch_bounds__(kEW) episode_count_kernel(const uint8_t *done, const int32_t *steps, int64_t B, int64_t groups,
                                                            int64_t rows, uint32_t *slots)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kEW / 64) + (threadIdx.x >> 6);      // (t, group) of this wavefront
    if (w >= rows * groups) return;
    const int64_t t = w / groups, b = (w % groups) * kEpisodeGroup + lane;
    const bool f = b < B && closes(done, steps, t, b, B);
    const unsigned long long m = __ballot(f);
    if (lane == 0) slots[w] = (uint32_t)__popcll(m);
}

// One workgroup: counts -> exclusive prefix in place (thread c owns a contiguous chunk), and the log's bookkeeping.
__global__ void __launch_bounds__(kScanW) episode_scan_kernel(uint32_t *slots, int64_t n, int64_t *head, int64_t capacity)
{
    __shared__ uint32_t wtot[kScanW / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t chunk = (n + kScanW - 1) / kScanW;
    const int64_t b = tid * chunk, e = b + chunk < n ? b + chunk : n;
    uint32_t s = 0;
    for (int64_t k = b; k < e; ++k) s += slots[k];
    uint32_t incl = s;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t off = 0;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    uint32_t run = off + incl - s;
    for (int64_t k = b; k < e; ++k) {
        const uint32_t c = slots[k];
        slots[k] = run;
        run += c;
    }
    if (tid == kScanW - 1) {                  // run = every closing step of this call
        const int64_t fill = head[0], want = fill + (int64_t)run;
        const int64_t now = want < capacity ? want : capacity;
        head[2] = fill;
        head[0] = now;
        head[1] += want - now;
    }
}

struct OpenEpisode {        // one lane's view: wavefront p holds plane p's sum; the counters are the same in all four
    double acc;
    int64_t cov_sum;
    int32_t cov_max, steps, ordinal;
};

// The record of a closing episode: wavefront p writes field p, wavefront 0 the rest; then the episode restarts.
__device__ __forceinline__ void close_episode(const EpisodeDevice &d, OpenEpisode &o, int p, int64_t b, int64_t slot)
{
    if (slot < d.log_capacity) {
        uavtrack_episode_record *r = d.log + slot;
        double *f = reinterpret_cast<double *>(r);
        f[p] = o.acc / (double)((int64_t)o.steps * d.N);
        if (p == 0) {
            r->average_covered = (double)o.cov_sum / (double)o.steps;
            r->max_covered = (double)o.cov_max;
            r->env = d.env_offset + b;
            r->steps = o.steps;
            r->ordinal = o.ordinal;
        }
    }
    o.acc = 0.0;
    o.cov_sum = 0;
    o.cov_max = 0;
    o.steps = 0;
    o.ordinal += 1;
}

__device__ __forceinline__ OpenEpisode load_episode(const EpisodeDevice &d, int p, int64_t b, bool live)
{
    OpenEpisode o = {0.0, 0, 0, 0, 0};
    if (live) {
        o.acc = d.acc[p * d.B + b];
        o.cov_sum = d.cov_sum[b];
        o.cov_max = d.cov_max[b];
        o.steps = d.steps[b];
        o.ordinal = d.ordinal[b];
    }
    return o;
}

__device__ __forceinline__ void store_episode(const EpisodeDevice &d, const OpenEpisode &o, int p, int64_t b, bool live)
{
    if (!live) return;
    d.acc[p * d.B + b] = o.acc;
    if (p == 0) {
        d.cov_sum[b] = o.cov_sum;
        d.cov_max[b] = o.cov_max;
        d.steps[b] = o.steps;
        d.ordinal[b] = o.ordinal;
    }
}

__global__ void __launch_bounds__(kEW) episode_fold_kernel(EpisodeDevice d, int64_t T, const int32_t *covered, const uint8_t *done)
{
    const int p = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = blockIdx.x, groups = gridDim.x, B = d.B;
    const int64_t b = g * kEpisodeGroup + lane;
    const bool live = b < B;
    OpenEpisode o = load_episode(d, p, b, live);
    __syncthreads();                          // wavefront 0 stores the counters the other three have just read
    const int64_t fill = done ? d.head[2] : 0;
    const unsigned long long below = (1ull << lane) - 1;
    for (int64_t t0 = 0; t0 < T; t0 += kFoldUnroll) {
        double x[kFoldUnroll];
        int32_t c[kFoldUnroll];
        uint8_t f[kFoldUnroll];
#pragma unroll
        for (int u = 0; u < kFoldUnroll; ++u) {
            const int64_t t = t0 + u;
            const bool in = live && t < T;
            x[u] = in ? d.step_sums[(t * kPlanes + p) * B + b] : 0.0;
            c[u] = in ? covered[t * B + b] : 0;
            f[u] = in && done ? done[t * B + b] : 0;
        }
#pragma unroll
        for (int u = 0; u < kFoldUnroll; ++u) {
            const int64_t t = t0 + u;
            if (t >= T) break;
            o.acc += x[u];                    // ascending t
            o.cov_sum += c[u];
            o.cov_max = o.steps == 0 || c[u] > o.cov_max ? c[u] : o.cov_max;
            o.steps += 1;
            const unsigned long long m = __ballot(f[u] != 0);
            if (f[u]) close_episode(d, o, p, b, fill + d.slots[t * groups + g] + __popcll(m & below));
        }
    }
    store_episode(d, o, p, b, live);
}

__global__ void __launch_bounds__(kEW) episode_close_kernel(EpisodeDevice d)
{
    const int p = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t g = blockIdx.x;
    const int64_t b = g * kEpisodeGroup + lane;
    const bool live = b < d.B;
    OpenEpisode o = load_episode(d, p, b, live);
    __syncthreads();
    const bool f = live && o.steps > 0;
    const unsigned long long m = __ballot(f);
    if (f) {
        close_episode(d, o, p, b, d.head[2] + d.slots[g] + __popcll(m & ((1ull << lane) - 1)));
        store_episode(d, o, p, b, true);
    }
}

// count + scan over `rows` rows of closing flags (done, or the open episodes that hold a step)
hipError_t launch_slots(const EpisodeDevice &d, int64_t rows, const uint8_t *done, hipStream_t stream)
{
    const int64_t groups = episode_groups(d.B), n = rows * groups;
    const unsigned blocks = (unsigned)((n + kEW / 64 - 1) / (kEW / 64));
    hipLaunchKernelGGL(episode_count_kernel, dim3(blocks), dim3(kEW), 0, stream, done, d.steps, d.B, groups, rows, d.slots);
    hipLaunchKernelGGL(episode_scan_kernel, dim3(1), dim3(kScanW), 0, stream, d.slots, n, d.head, d.log_capacity);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_episode_add(const EpisodeDevice &d, int64_t T, const float *reward, const float *terms,
                              const int32_t *covered, const uint8_t *done, hipStream_t stream)
{
    int64_t E = kStageFloats / d.N;
    if (E > kEpisodeGroup) E = kEpisodeGroup;
    if (E > d.B) E = d.B;
    const int64_t tiles = (d.B + E - 1) / E;
    const int n = (int)(E * d.N), plane_floats = n + (n >> 5) + 1;
    hipLaunchKernelGGL(episode_step_sums_kernel, dim3((unsigned)(T * tiles)), dim3(kEW),
                       (size_t)kPlanes * plane_floats * sizeof(float), stream, reward, terms, d.step_sums, d.B, d.N, (int)E,
                       (int)tiles, plane_floats);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess && done) e = launch_slots(d, T, done, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(episode_fold_kernel, dim3((unsigned)episode_groups(d.B)), dim3(kEW), 0, stream, d, T, covered, done);
    return hipGetLastError();
}

hipError_t launch_episode_close(const EpisodeDevice &d, hipStream_t stream)
{
    hipError_t e = launch_slots(d, 1, nullptr, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(episode_close_kernel, dim3((unsigned)episode_groups(d.B)), dim3(kEW), 0, stream, d);
    return hipGetLastError();
}

}  // namespace uavtrack

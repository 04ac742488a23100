// actor_pack_kernel.hip -- pack_actor_blob (actor.h) restated on the device, for uavtrack_publish_actor_weights and
// uavtrack_learner_publish_actor: the rollout actor's weight blob written straight from fp32 device tensors in torch
// layouts, stream-ordered, with no allocation and no synchronisation, bitwise identical to the host pack of the same
// weights.  Two launches:
//   actor_pack_bounds_kernel   one workgroup: the fp64 bounds in the host's order -- per unit |b1| + the sequential sum over
//                              k = 0..11 of |w1[u][k]| xb[k] (one thread per unit), their maximum, the maxima of |W1|, |b1|
//                              and |W2| (maxima drop NaN, as std::fmax, and are free of order) -- the block scales T1, T2
//                              (actor_pow2_below, the host's formula), then per action |b2[q]| + the sequential sum over u of
//                              |w2[q][u]| 60000 / T1 (one thread per action, W2 staged through LDS a chunk of units at a
//                              time), and the 128 header floats: 1 / (T1 T2), the softmax-guard flag, b2, zeros;
//   actor_pack_frags_kernel    one wavefront per 32-unit tile: every fragment word of the tile, in put()'s lane and element
//                              order, as 16-byte vector stores (zeros at u >= H and q >= A).
// Every word of the blob is written on every call, so nothing of an earlier set of weights survives.  -ffp-contract=off
// (Makefile) keeps each product and sum rounded on its own, as on the host.  The one place the two can part: log2 is the
// host's libm in pack_actor_blob and the device math library here; at a ratio target / bound within an ulp or two of a
// power of two their floors may differ by one, and the blobs then differ by that factor of two in one scale.

#include "actor.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kPackThreads = 1024;                    // the bounds kernel's one workgroup: 16 wavefronts
constexpr int kPackChunk = 256;                       // units of W2 staged in LDS per pass of the logit bound
constexpr int kPackStride = kPackChunk + 1;           // (one float of padding: the action threads read down a column)

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(kPackThreads) void actor_pack_bounds_kernel(ActorPackArgs a)
{
    __shared__ float w2s[48 * kPackStride];
    __shared__ double red[3][kPackThreads / 64];
    __shared__ double scale[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, H = a.H, A = a.A;
    double act = 0.0, w1max = 0.0, w2max = 0.0;
    for (int u = tid; u < H; u += kPackThreads) {
        double s = fabs((double)a.b1[u]);
        w1max = fmax(w1max, s);
        for (int k = 0; k < kActorObs; ++k) {
            const double w = fabs((double)a.w1[(size_t)u * kActorObs + k]);
            s += w * a.xb[k];
            w1max = fmax(w1max, w);
        }
        act = fmax(act, s);
    }
    for (size_t i = tid; i < (size_t)A * H; i += kPackThreads) w2max = fmax(w2max, fabs((double)a.w2[i]));
    act = wave_max(act);
    w1max = wave_max(w1max);
    w2max = wave_max(w2max);
    if (lane == 0) {
        red[0][wave] = act;
        red[1][wave] = w1max;
        red[2][wave] = w2max;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kPackThreads / 64; ++w) {
            act = fmax(act, red[0][w]);
            w1max = fmax(w1max, red[1][w]);
            w2max = fmax(w2max, red[2][w]);
        }
        const double T1 = fmin(actor_pow2_below(act, 512.0), actor_pow2_below(w1max, 16384.0));
        const double T2 = actor_pow2_below(w2max, 16384.0);
        scale[0] = T1;
        scale[1] = T2;
        a.scales[0] = T1;
        a.scales[1] = T2;
    }
    __syncthreads();
    const double T1 = scale[0], T2 = scale[1];
    // the logit bound: thread q < A sums its row in the host's order, W2 passing through LDS kPackChunk units at a time
    const double cap = kActorCap / T1;
    double l = tid < A ? fabs((double)a.b2[tid]) : 0.0;
    for (int u0 = 0; u0 < H; u0 += kPackChunk) {
        const int n = H - u0 < kPackChunk ? H - u0 : kPackChunk;
        __syncthreads();                                      // (the previous chunk has been read)
        for (int i = tid; i < A * kPackChunk; i += kPackThreads) {
            const int q = i / kPackChunk, u = i % kPackChunk;
            if (u < n) w2s[q * kPackStride + u] = a.w2[(size_t)q * H + u0 + u];
        }
        __syncthreads();
        if (tid < A)
            for (int u = 0; u < n; ++u) l += fabs((double)w2s[tid * kPackStride + u]) * cap;
    }
    if (wave == 0) {
        const double lmax = wave_max(tid < A ? l : 0.0);      // (A <= 48: one wavefront holds every action)
        // the header: 1 / (T1 T2), the guard flag, b2 (bit for bit), zeros
        for (int i = lane; i < kActorHeaderFloats; i += 64) {
            float v = 0.0f;
            if (i == 0) v = (float)(1.0 / (T1 * T2));
            else if (i == 1) v = !(lmax < 268435456.0) ? 1.0f : 0.0f;
            else if (i >= kActorB2Offset && i < kActorB2Offset + A) v = a.b2[i - kActorB2Offset];
            a.blob[i] = v;
        }
    }
}

// one wavefront per 32-unit tile `a`: lane l holds row l % 32 and k-half l >> 5 of every fragment of the tile (put())
__global__ __launch_bounds__(64) void actor_pack_frags_kernel(ActorPackArgs p)
{
    const int a = blockIdx.x, lane = threadIdx.x, row = lane & 31, kh = lane >> 5, H = p.H, A = p.A;
    const int FT = actor_frags_per_tile(p.at);
    const double T1 = p.scales[0], T2 = p.scales[1];
    uint4 *frag = reinterpret_cast<uint4 *>(p.blob + kActorHeaderFloats) + (size_t)a * FT * 64 + lane;
    auto store = [&](int f, const uint32_t (&w)[8]) {         // hi words into fragment f, lo words into f + 1
        uint4 hi, lo;
        hi.x = (w[0] & 0xFFFFu) | (w[1] << 16); lo.x = (w[0] >> 16) | (w[1] & 0xFFFF0000u);
        hi.y = (w[2] & 0xFFFFu) | (w[3] << 16); lo.y = (w[2] >> 16) | (w[3] & 0xFFFF0000u);
        hi.z = (w[4] & 0xFFFFu) | (w[5] << 16); lo.z = (w[4] >> 16) | (w[5] & 0xFFFF0000u);
        hi.w = (w[6] & 0xFFFFu) | (w[7] << 16); lo.w = (w[6] >> 16) | (w[7] & 0xFFFF0000u);
        frag[(size_t)f * 64] = hi;
        frag[(size_t)(f + 1) * 64] = lo;
    };
    uint32_t w[8];
    // layer 1: unit 32 a + row, k = 8 kh + j: inputs 0..11, then the bias on the constant input, then zeros
    const int u = 32 * a + row;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = 8 * kh + j;
        float v = 0.0f;
        if (u < H) v = k < kActorObs ? p.w1[(size_t)u * kActorObs + k] : (k == kActorObs ? p.b1[u] : 0.0f);
        w[j] = actor_split_word(T1, v);
    }
    store(0, w);
    // layer 2, action tile t, k-step half: action 32 t + row against the unit the B operand's lane holds at k = 8 kh + j
    for (int t = 0; t < p.at; ++t)
        for (int half = 0; half < 2; ++half) {
            const int q = 32 * t + row;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int unit = 32 * a + actor_unit_of(8 * half + j, kh);
                const float v = (unit < H && q < A) ? p.w2[(size_t)q * H + unit] : 0.0f;
                w[j] = actor_split_word(T2, v);
            }
            store(2 + 4 * t + 2 * half, w);
        }
}

}  // namespace

hipError_t launch_actor_pack(const ActorPackArgs &a, hipStream_t st)
{
    hipLaunchKernelGGL(actor_pack_bounds_kernel, dim3(1), dim3(kPackThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(actor_pack_frags_kernel, dim3(actor_blocks(a.H)), dim3(64), 0, st, a);
    return hipGetLastError();
}

}  // namespace uavtrack

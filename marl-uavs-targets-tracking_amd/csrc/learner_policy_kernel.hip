// learner_policy_kernel.hip -- the actor alone: log pi(a | s) of rows with the learner's actor as it stands when the
// launch runs (uavtrack_learner_log_probs, _log_probs_window), and the truncated importance ratios of a batch against
// a per-slot store of behaviour log-probabilities, fused with that forward (uavtrack_learner_ratio_weights).
//
// One kernel, learner_policy_kernel, modelled on learner_values_kernel: one lane owns two rows (i and i + kPW of the
// workgroup's chunk of 2 kPW), 24 inputs from six 16-byte loads and 2 x kA logit accumulators in registers.  The actor's
// 13 H + A H words are wavefront-uniform; the workgroup copies them into LDS once, one record per hidden unit
// {W1a[j][0..11], b1a[j], W2a[0..A-1][j], zeros} of 13 + kA words padded to a 16-byte multiple (kA: A rounded up to 12,
// 16, 32 or 48; at most 64 words, 64 KiB at H = 256), and every lane reads a record through the same address.
// The chains are the gradient kernel's, explicit fmaf in its order, nothing reassociated:
//   p_j = b1a[j]; for k = 0 .. 11: p_j = fmaf(W1a[j][k], s[k], p_j); h_j = fmaxf(p_j, 0)
//   z_o = b2a[o]; for j = 0 .. H - 1: z_o = fmaf(W2a[o][j], h_j, z_o)
//   log p_a = (z_a - max) - logf(sum_o expf(z_o - max)),  the sum in ascending o
// the logits form of the regularised update: finite for every finite logit vector.  A row's chain sees only that row's
// inputs and the parameters, so its bits do not depend on the lane, the workgroup or the launch that carries it.
// No status word: a slot outside [0, capacity) or an action outside [0, A) gives NaN, which the update behind a ratio
// refuses as a bad weight.

#include "learner_policy.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kPW = 256;          // threads per workgroup

constexpr int policy_rec_words(int kA) { return (13 + kA + 3) / 4 * 4; }

__device__ __forceinline__ void load_state(float (&x)[12], const float *src)
{
    const float4 *s = reinterpret_cast<const float4 *>(src);
    const float4 a = s[0], b = s[1], c = s[2];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
}

// the slot of row i, or -1 where it lies outside the store
__device__ __forceinline__ int64_t slot_of(const PolicyLaunch &q, int64_t i)
{
    if (q.first >= 0) return (q.first + i) % q.capacity;
    const int64_t src = q.idx ? q.idx[i] : i;
    return src >= 0 && src < q.capacity ? src : -1;
}

// log p_a from the logits z[0..A-1]; a in [0, A)
template <int kA>
__device__ __forceinline__ float log_prob(const float (&z)[kA], int A, int a)
{
    float m = z[0], za = z[0];
#pragma unroll
    for (int o = 1; o < kA; ++o)
        if (o < A) {
            m = fmaxf(m, z[o]);
            za = o == a ? z[o] : za;
        }
    float sum = 0.0f;
#pragma unroll
    for (int o = 0; o < kA; ++o)
        if (o < A) sum += expf(z[o] - m);
    return (za - m) - logf(sum);
}

// what becomes of one row's log p: the store of a log-probability call, the ratio and the weight of a ratio call
__device__ __forceinline__ void finish_row(const PolicyLaunch &q, int64_t i, int64_t src, float lp)
{
    if (q.log_probs) q.log_probs[q.first >= 0 ? src : i] = lp;
    if (!q.log_mu) return;
    float rho = NAN;
    if (src >= 0) {
        const float lm = q.log_mu[src];
        if (lm <= 0.0f && lp == lp) rho = fminf(q.rho_bar, expf(lp - lm));
    }
    q.weights_out[i] = (q.weights_in ? q.weights_in[i] : 1.0f) * rho;
    if (q.rho_out) q.rho_out[i] = rho;
}

template <int kA>
__global__ void __launch_bounds__(kPW) learner_policy_kernel(const float *params, LearnerLayout L, PolicyLaunch q)
{
    constexpr int RW = policy_rec_words(kA);
    extern __shared__ __attribute__((aligned(16))) float rec[];
    const int tid = threadIdx.x, H = L.H, A = L.A;
    const float *W1a = params + L.a_w1, *b1a = params + L.a_b1, *W2a = params + L.a_w2, *b2a = params + L.a_b2;
    for (int e = tid; e < H * RW; e += kPW) {
        const int j = e / RW, k = e - j * RW;
        rec[e] = k < 12 ? W1a[j * 12 + k] : (k == 12 ? b1a[j] : (k - 13 < A ? W2a[(k - 13) * H + j] : 0.0f));
    }
    float bias[kA];
#pragma unroll
    for (int o = 0; o < kA; ++o) bias[o] = o < A ? b2a[o] : 0.0f;
    __syncthreads();
    const int64_t chunk = 2 * kPW;
    for (int64_t base = (int64_t)blockIdx.x * chunk; base < q.n; base += (int64_t)gridDim.x * chunk) {
        const int64_t i0 = base + tid, i1 = i0 + kPW;
        const int64_t s0 = i0 < q.n ? slot_of(q, i0) : -1, s1 = i1 < q.n ? slot_of(q, i1) : -1;
        float x0[12], x1[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { x0[k] = 0.0f; x1[k] = 0.0f; }
        int a0 = -1, a1 = -1;
        if (s0 >= 0) { load_state(x0, q.states + s0 * 12); a0 = q.actions[s0]; }
        if (s1 >= 0) { load_state(x1, q.states + s1 * 12); a1 = q.actions[s1]; }
        float z0[kA], z1[kA];
#pragma unroll
        for (int o = 0; o < kA; ++o) { z0[o] = bias[o]; z1[o] = bias[o]; }
#pragma unroll 1
        for (int j = 0; j < H; ++j) {
            const float4 *r = reinterpret_cast<const float4 *>(rec + j * RW);
            float w[RW];
#pragma unroll
            for (int v = 0; v < RW / 4; ++v) {
                const float4 t = r[v];
                w[4 * v] = t.x; w[4 * v + 1] = t.y; w[4 * v + 2] = t.z; w[4 * v + 3] = t.w;
            }
            float p0 = w[12], p1 = w[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                p0 = fmaf(w[k], x0[k], p0);
                p1 = fmaf(w[k], x1[k], p1);
            }
            const float h0 = fmaxf(p0, 0.0f), h1 = fmaxf(p1, 0.0f);
#pragma unroll
            for (int o = 0; o < kA; ++o) {
                z0[o] = fmaf(w[13 + o], h0, z0[o]);
                z1[o] = fmaf(w[13 + o], h1, z1[o]);
            }
        }
        if (i0 < q.n) finish_row(q, i0, s0, a0 >= 0 && a0 < A ? log_prob<kA>(z0, A, a0) : NAN);
        if (i1 < q.n) finish_row(q, i1, s1, a1 >= 0 && a1 < A ? log_prob<kA>(z1, A, a1) : NAN);
    }
}

template <int kA>
hipError_t launch_tier(const LearnerDevice &d, const PolicyLaunch &q, unsigned blocks, hipStream_t st)
{
    static_assert(kLearnerMaxHidden * policy_rec_words(kA) * sizeof(float) <= 64 * 1024, "the actor's records fit LDS");
    const size_t lds = (size_t)d.L.H * policy_rec_words(kA) * sizeof(float);
    hipLaunchKernelGGL(learner_policy_kernel<kA>, dim3(blocks), dim3(kPW), lds, st, d.params, d.L, q);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_learner_policy(const LearnerDevice &d, const PolicyLaunch &q, hipStream_t st)
{
    static_assert(kLearnerMaxActions <= 48, "the widest tier holds every action");
    int64_t blocks = (q.n + 2 * kPW - 1) / (2 * kPW);
    if (blocks > 1024) blocks = 1024;
    const int A = d.L.A;
    if (A <= 12) return launch_tier<12>(d, q, (unsigned)blocks, st);
    if (A <= 16) return launch_tier<16>(d, q, (unsigned)blocks, st);
    if (A <= 32) return launch_tier<32>(d, q, (unsigned)blocks, st);
    return launch_tier<48>(d, q, (unsigned)blocks, st);
}

}  // namespace uavtrack

// pmi_train_kernel.hip -- PMINetwork.train_pmi (PMINet.py:74-100) on the device: b2 // bs mini-batch steps, each two
// train-mode forwards (input_1_2, input_1_3), CustomLoss, the backward pass through both and a torch.optim.Adam step.
//
// One call is a chain of stream-ordered launches, none of which synchronises or allocates:
//   pmi_begin_kernel          every index triple of the call checked (a bad one turns the whole call into a no-op),
//                             the |loss| accumulator cleared;
// then per mini-batch step:
//   pmi_branch_fwd_kernel     one wavefront per branch feature (3H): rows gathered through the index triples, the
//                             branch Linear, batch mean / biased variance, normalise, ReLU; running statistics;
//   pmi_gemm_kernel           fc1: a 32 x 32-tiled fp32 GEMM over LDS slices, 2 x 2 outputs per thread;
//   pmi_bn1_fwd_kernel        one wavefront per fc1 output (H): bn1 statistics, normalise, ReLU; running statistics;
//   pmi_head_kernel           one workgroup of 1024 threads: fc2, the softplus loss, dL/d(output), fc2.bias
//                             gradient, |loss|, the Adam step and num_batches_tracked counters;
//   pmi_bn1_bwd_kernel        one wavefront per fc1 output: the train-mode bn1 backward -> dL/d(fc1 output),
//                             gradients of fc2.weight, fc1.bias, bn1.weight, bn1.bias;
//   pmi_gemm_kernel (x 2)     fc1.weight's gradient, and dL/d(branch output) masked by the branch ReLU;
//   pmi_branch_bwd_kernel     one wavefront per branch feature: the train-mode BN backward, the branch gradients;
//   pmi_adam_kernel           per trainable element: Adam on the gradient the kernels above wrote (zero_grad
//                             semantics: every gradient is rewritten each step);
// and pmi_finalize_kernel: avg_loss, the refusal count.
// uavtrack_pmi_trainer_train_many runs the same chain on rows that pmi_select_kernel first gathers from a list of
// histories into the trainer's scratch (the step kernels' arithmetic does not depend on where a row came from);
// uavtrack_pmi_trainer_select is that gather alone, for one participant's span of a timeline.
// Every sum over the batch is owned by one wavefront (lanes over rows, a fixed xor-butterfly reduction) or one thread,
// so there are no float atomics and two identical calls give bitwise identical results.  Both forwards of a step live
// in the same wavefront, which applies their running-statistics updates in the reference's order.
// Intermediates are stored feature-major ([side][feature][row]) so the lanes of a wavefront read consecutive rows.

#include "pmi_train.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kWG = 256;                 // threads per workgroup; the column kernels run one feature per wavefront
constexpr int kWavesPerWG = kWG / 64;
constexpr float kBnEps = 1e-5f;          // BatchNorm1d defaults (PMINet.py:30-37)
constexpr float kBnMomentum = 0.1f;

struct StepArgs {
    PmiTrainLayout L;
    const float *rows;
    const int64_t *t_idx, *u_idx;        // the call's triples; this step's start at row0
    int64_t n_uav, row0;
    int B;                               // batch rows
    int step;                            // mini-batch number within the call
    float *state, *grad;
    int64_t *nbt, *steps;
    float *xh0, *a0, *da0, *xh1, *a1, *dz1, *inv0, *inv1, *go, *acc;
    float *losses, *outputs;             // nullable
    const int *status;
};

__device__ __forceinline__ float wave_sum(float v)
{
    // xor butterfly: every lane ends with the same value, in an order fixed by the lane pattern
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ const float *gathered_row(const StepArgs &a, int side, int i)
{
    const int64_t g = a.row0 + i;
    return a.rows + (a.t_idx[g] * a.n_uav + a.u_idx[2 * g + side]) * 12;
}

__device__ __forceinline__ float softplus(float x) { return fmaxf(x, 0.0f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float sigmoid(float x)
{
    const float e = expf(-fabsf(x));
    return x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
}

// one BatchNorm1d's running statistics after a forward (torch: running = (1 - momentum) running + momentum batch,
// the variance unbiased)
__device__ __forceinline__ void update_running(float *rm, float *rv, float mean, float var_biased, int B)
{
    *rm = (1.0f - kBnMomentum) * *rm + kBnMomentum * mean;
    *rv = (1.0f - kBnMomentum) * *rv + kBnMomentum * (var_biased * (float)B / (float)(B - 1));
}

constexpr int kRegRows = 8;              // rows per lane a column kernel keeps in registers (batches up to 512)

// The statistics of one feature over the batch, z_of(i) giving its pre-BN value in row i, then normalise + ReLU:
// xh[i] = (z - mean) * inv, act[i] = max(gamma xh + beta, 0).  Returns (mean, biased var, inv).  Batches up to
// 64 x kRegRows rows stay in registers; larger ones pass through xh.  Both paths add in the same order.
template <typename ZF>
__device__ __forceinline__ float3 bn_forward_column(ZF z_of, float *xh, float *act, int B, int lane, float gamma,
                                                    float beta)
{
    if (B <= 64 * kRegRows) {
        float z[kRegRows], s = 0.0f;
#pragma unroll
        for (int r = 0; r < kRegRows; ++r) {
            const int i = lane + 64 * r;
            z[r] = i < B ? z_of(i) : 0.0f;
            s += z[r];
        }
        const float mean = wave_sum(s) / (float)B;
        float q = 0.0f;
#pragma unroll
        for (int r = 0; r < kRegRows; ++r)
            if (lane + 64 * r < B) { const float d = z[r] - mean; q = fmaf(d, d, q); }
        const float var = wave_sum(q) / (float)B;
        const float inv = 1.0f / sqrtf(var + kBnEps);
#pragma unroll
        for (int r = 0; r < kRegRows; ++r) {
            const int i = lane + 64 * r;
            if (i < B) {
                const float x = (z[r] - mean) * inv;
                xh[i] = x;
                act[i] = fmaxf(fmaf(gamma, x, beta), 0.0f);
            }
        }
        return make_float3(mean, var, inv);
    }
    float s = 0.0f;
    for (int i = lane; i < B; i += 64) { const float z = z_of(i); xh[i] = z; s += z; }
    const float mean = wave_sum(s) / (float)B;
    float q = 0.0f;
    for (int i = lane; i < B; i += 64) { const float d = xh[i] - mean; q = fmaf(d, d, q); }
    const float var = wave_sum(q) / (float)B;
    const float inv = 1.0f / sqrtf(var + kBnEps);
    for (int i = lane; i < B; i += 64) {
        const float x = (xh[i] - mean) * inv;
        xh[i] = x;
        act[i] = fmaxf(fmaf(gamma, x, beta), 0.0f);
    }
    return make_float3(mean, var, inv);
}

__global__ void pmi_begin_kernel(const int64_t *t_idx, const int64_t *u_idx, int64_t b2, int64_t T, int64_t n_uav,
                                 int *status, float *acc)
{
    int bad = 0;
    for (int64_t g = threadIdx.x; g < b2; g += blockDim.x) {
        const int64_t t = t_idx[g], u0 = u_idx[2 * g], u1 = u_idx[2 * g + 1];
        if (t < 0 || t >= T || u0 < 0 || u0 >= n_uav || u1 < 0 || u1 >= n_uav) bad = 1;
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) { *status = bad; *acc = 0.0f; }
}

__global__ void __launch_bounds__(kWG) pmi_branch_fwd_kernel(StepArgs a)
{
    if (*a.status) return;
    const int H = a.L.H, B = a.B, lane = threadIdx.x & 63;
    const int j = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (j >= 3 * H) return;                                   // whole wavefronts only: no workgroup barrier follows
    const int br = j / H, jj = j - br * H;
    const int K = br == 0 ? 5 : (br == 1 ? 4 : 3), k0 = br == 0 ? 0 : (br == 1 ? 5 : 9);
    const int *so = a.L.soff + br * 6;
    const float *W = a.state + so[0] + jj * K;
    const float bias = a.state[so[1] + jj], gamma = a.state[so[2] + jj], beta = a.state[so[3] + jj];
    for (int s = 0; s < 2; ++s) {
        float *xh = a.xh0 + ((size_t)s * 3 * H + j) * B;
        float *act = a.a0 + ((size_t)s * 3 * H + j) * B;
        auto z_of = [&](int i) {
            const float *x = gathered_row(a, s, i) + k0;
            float z = bias;
            for (int k = 0; k < K; ++k) z = fmaf(W[k], x[k], z);
            return z;
        };
        const float3 st = bn_forward_column(z_of, xh, act, B, lane, gamma, beta);
        if (lane == 0) {
            a.inv0[s * 3 * H + j] = st.z;
            update_running(a.state + so[4] + jj, a.state + so[5] + jj, st.x, st.y, B);
        }
    }
}

// One operand of the tiled GEMM: element (x, y) at p + idx(x) + idx(y), where an index may be a (side, row) pair
// j = side * seg + row of the feature-major scratch: idx(j) = (j / seg) * side_stride + (j % seg) * stride.
struct Opnd {
    const float *p;
    int64_t sx, sy;                      // strides of x and y
    int segx, segy;                      // 0: plain index; else rows per side
    int64_t ssx, ssy;                    // side strides
    __device__ __forceinline__ int64_t idx(int j, int64_t st, int seg, int64_t ss) const
    {
        if (!seg) return (int64_t)j * st;
        const int q = j / seg;
        return (int64_t)q * ss + (int64_t)(j - q * seg) * st;
    }
    __device__ __forceinline__ int64_t at(int x, int y) const { return idx(x, sx, segx, ssx) + idx(y, sy, segy, ssy); }
};

constexpr int kTM = 16, kTN = 16, kTK = 128;  // output tile and reduction slice of pmi_gemm_kernel

enum GemmEpilogue { kStore = 0, kAddBias = 1, kReluMask = 2 };

// C(m, n) = sum_r A(m, r) B(r, n) over an M x N grid of 16 x 16 tiles, one output per thread, from LDS slices of 128
// reductions.  The work is small and latency-bound: small tiles spread it over more CUs (32 x 32 tiles with 2 x 2
// outputs per thread kept the fc1 forward on 32 workgroups), and each slice costs one round trip to memory.  Every
// output is one thread's sum in r order, so the result is independent of the launch.  Epilogues: kAddBias adds
// bias[m]; kReluMask zeroes the outputs whose mask (addressed like C) is <= 0.
__global__ void __launch_bounds__(kWG) pmi_gemm_kernel(Opnd A, Opnd Bo, Opnd C, int M, int N, int R, int epilogue,
                                                       const float *bias, Opnd mask, const int *status)
{
    __shared__ float As[kTK][kTM + 1];
    __shared__ float Bs[kTK][kTN + 1];
    if (*status) return;
    const int tid = threadIdx.x;
    const int m0 = blockIdx.y * kTM, n0 = blockIdx.x * kTN;
    const int tm = tid / kTN, tn = tid - tm * kTN;
    float acc = 0.0f;
    constexpr int kLA = kTM * kTK / kWG, kLB = kTK * kTN / kWG;   // slice elements per thread
    for (int r0 = 0; r0 < R; r0 += kTK) {
        // every load of the slice is issued before the first is waited for: one memory round trip per slice
        float va[kLA], vb[kLB];
#pragma unroll
        for (int q = 0; q < kLA; ++q) {
            const int e = tid + q * kWG, mm = e / kTK, rr = e - mm * kTK;   // A: consecutive threads along r
            const int m = m0 + mm, r = r0 + rr;
            va[q] = (m < M && r < R) ? A.p[A.at(m, r)] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kLB; ++q) {
            const int e = tid + q * kWG, rr = e / kTN, nn = e - rr * kTN;   // B: consecutive threads along n
            const int n = n0 + nn, r = r0 + rr;
            vb[q] = (n < N && r < R) ? Bo.p[Bo.at(r, n)] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kLA; ++q) {
            const int e = tid + q * kWG, mm = e / kTK;
            As[e - mm * kTK][mm] = va[q];
        }
#pragma unroll
        for (int q = 0; q < kLB; ++q) {
            const int e = tid + q * kWG, rr = e / kTN;
            Bs[rr][e - rr * kTN] = vb[q];
        }
        __syncthreads();
#pragma unroll 16
        for (int rr = 0; rr < kTK; ++rr) acc = fmaf(As[rr][tm], Bs[rr][tn], acc);
        __syncthreads();
    }
    const int m = m0 + tm, n = n0 + tn;
    if (m >= M || n >= N) return;
    float v = acc;
    if (epilogue == kAddBias) v += bias[m];
    else if (epilogue == kReluMask && !(mask.p[mask.at(m, n)] > 0.0f)) v = 0.0f;
    const_cast<float *>(C.p)[C.at(m, n)] = v;
}

// bn1 over fc1's outputs (already in xh1 as pre-BN values): one wavefront per feature, both sides
__global__ void __launch_bounds__(kWG) pmi_bn1_fwd_kernel(StepArgs a)
{
    if (*a.status) return;
    const int H = a.L.H, B = a.B, lane = threadIdx.x & 63;
    const int c = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (c >= H) return;
    const int *so = a.L.soff + 3 * 6;
    const float gamma = a.state[so[2] + c], beta = a.state[so[3] + c];
    for (int s = 0; s < 2; ++s) {
        float *xh = a.xh1 + ((size_t)s * H + c) * B;
        float *act = a.a1 + ((size_t)s * H + c) * B;
        const float3 st = bn_forward_column([&](int i) { return xh[i]; }, xh, act, B, lane, gamma, beta);
        if (lane == 0) {
            a.inv1[s * H + c] = st.z;
            update_running(a.state + so[4] + c, a.state + so[5] + c, st.x, st.y, B);
        }
    }
}

constexpr int kHeadThreads = 1024;       // pmi_head_kernel: four threads per output row
constexpr int kHeadSplit = 4;

__global__ void __launch_bounds__(kHeadThreads) pmi_head_kernel(StepArgs a)
{
    __shared__ float part[kHeadThreads];
    __shared__ float red[2][kHeadThreads / kHeadSplit];
    const int H = a.L.H, B = a.B, tid = threadIdx.x;
    if (*a.status) {
        if (tid == 0 && a.losses) a.losses[a.step] = NAN;
        return;
    }
    const float *w2 = a.state + a.L.soff[24];
    const float b2 = a.state[a.L.soff[25]];
    const int q = tid % kHeadSplit, slot = tid / kHeadSplit;
    float lsum = 0.0f, gsum = 0.0f;
    for (int r0 = 0; r0 < 2 * B; r0 += kHeadThreads / kHeadSplit) {
        // fc2: thread q of a row sums the features c = q, q + 4, ..., eight loads in flight at a time
        const int r = r0 + slot;
        float p = 0.0f;
        if (r < 2 * B) {
            const int s = r >= B, i = r - s * B;
            const float *act = a.a1 + (size_t)s * H * B + i;
            int c = q;
            for (; c + 7 * kHeadSplit < H; c += 8 * kHeadSplit) {
                float x[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) x[u] = act[(size_t)(c + u * kHeadSplit) * B];
#pragma unroll
                for (int u = 0; u < 8; ++u) p = fmaf(w2[c + u * kHeadSplit], x[u], p);
            }
            for (; c < H; c += kHeadSplit) p = fmaf(w2[c], act[(size_t)c * B], p);
        }
        part[tid] = p;
        __syncthreads();
        if (q == 0 && r < 2 * B) {
            const int s = r >= B;
            float o = b2;
            for (int u = 0; u < kHeadSplit; ++u) o += part[tid + u];
            // CustomLoss: softplus(-o12) + softplus(o13), mean over the batch
            const float term = s == 0 ? softplus(-o) : softplus(o);
            const float g = (s == 0 ? -sigmoid(-o) : sigmoid(o)) / (float)B;
            a.go[r] = g;
            if (a.outputs) a.outputs[(size_t)a.step * 2 * B + r] = o;
            lsum += term;
            gsum += g;
        }
        __syncthreads();
    }
    if (q == 0) { red[0][slot] = lsum; red[1][slot] = gsum; }
    __syncthreads();
    for (int off = kHeadThreads / kHeadSplit / 2; off > 0; off >>= 1) {
        if (tid < off) { red[0][tid] += red[0][tid + off]; red[1][tid] += red[1][tid + off]; }
        __syncthreads();
    }
    if (tid == 0) {
        const float loss = fabsf(red[0][0] / (float)B);
        *a.acc += loss;
        if (a.losses) a.losses[a.step] = loss;
        a.grad[a.L.poff[17]] = red[1][0];                     // fc2.bias
        for (int t = 0; t < kPmiTrainTensors; ++t) a.steps[t] += 1;
        for (int b = 0; b < kPmiBlocks; ++b) a.nbt[b] += 2;   // two forwards per step
    }
}

// the train-mode BatchNorm backward of one feature over the batch, one side:
// dz = gamma inv (dy - mean(dy) - xh mean(dy xh)) with dy produced by dy_of(i).  Returns (sum dy, sum dy xh) and
// hands each row's dz to sink(i, dz).  Batches up to 64 x kRegRows rows keep dy and xh in registers.
template <typename DY, typename SINK>
__device__ __forceinline__ float2 bn_backward_column(const float *xh, int B, int lane, float gamma, float inv, DY dy_of,
                                                     SINK sink)
{
    float sdy = 0.0f, sdx = 0.0f;
    if (B <= 64 * kRegRows) {
        float dy[kRegRows], x[kRegRows];
#pragma unroll
        for (int r = 0; r < kRegRows; ++r) {
            const int i = lane + 64 * r;
            dy[r] = i < B ? dy_of(i) : 0.0f;
            x[r] = i < B ? xh[i] : 0.0f;
            sdy += dy[r];
            sdx = fmaf(dy[r], x[r], sdx);
        }
        sdy = wave_sum(sdy);
        sdx = wave_sum(sdx);
        const float mdy = sdy / (float)B, mdx = sdx / (float)B, gi = gamma * inv;
#pragma unroll
        for (int r = 0; r < kRegRows; ++r)
            if (lane + 64 * r < B) sink(lane + 64 * r, gi * (dy[r] - mdy - x[r] * mdx));
        return make_float2(sdy, sdx);
    }
    for (int i = lane; i < B; i += 64) { const float dy = dy_of(i); sdy += dy; sdx = fmaf(dy, xh[i], sdx); }
    sdy = wave_sum(sdy);
    sdx = wave_sum(sdx);
    const float mdy = sdy / (float)B, mdx = sdx / (float)B, gi = gamma * inv;
    for (int i = lane; i < B; i += 64) sink(i, gi * (dy_of(i) - mdy - xh[i] * mdx));
    return make_float2(sdy, sdx);
}

__global__ void __launch_bounds__(kWG) pmi_bn1_bwd_kernel(StepArgs a)
{
    if (*a.status) return;
    const int H = a.L.H, B = a.B, lane = threadIdx.x & 63;
    const int c = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (c >= H) return;
    const int *so = a.L.soff + 3 * 6;
    const float gamma = a.state[so[2] + c], w2 = a.state[a.L.soff[24] + c];
    float gw2 = 0.0f, gb1 = 0.0f, gg = 0.0f, gbe = 0.0f;
    for (int s = 0; s < 2; ++s) {
        const float *xh = a.xh1 + ((size_t)s * H + c) * B;
        const float *act = a.a1 + ((size_t)s * H + c) * B;
        const float *go = a.go + (size_t)s * B;
        float *dz = a.dz1 + ((size_t)s * H + c) * B;
        float pw = 0.0f, pb = 0.0f;
        for (int i = lane; i < B; i += 64) pw = fmaf(go[i], act[i], pw);
        const float2 r = bn_backward_column(
            xh, B, lane, gamma, a.inv1[s * H + c],
            [&](int i) { return act[i] > 0.0f ? go[i] * w2 : 0.0f; },
            [&](int i, float v) { dz[i] = v; pb += v; });
        gw2 += wave_sum(pw);
        gb1 += wave_sum(pb);
        gbe += r.x;
        gg += r.y;
    }
    if (lane == 0) {
        a.grad[a.L.poff[16] + c] = gw2;                       // fc2.weight
        a.grad[a.L.poff[13] + c] = gb1;                       // fc1.bias
        a.grad[a.L.poff[14] + c] = gg;                        // bn1.weight
        a.grad[a.L.poff[15] + c] = gbe;                       // bn1.bias
    }
}

__global__ void __launch_bounds__(kWG) pmi_branch_bwd_kernel(StepArgs a)
{
    if (*a.status) return;
    const int H = a.L.H, B = a.B, lane = threadIdx.x & 63;
    const int j = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (j >= 3 * H) return;
    const int br = j / H, jj = j - br * H;
    const int K = br == 0 ? 5 : (br == 1 ? 4 : 3), k0 = br == 0 ? 0 : (br == 1 ? 5 : 9);
    const int *so = a.L.soff + br * 6;
    const int *po = a.L.poff + br * 4;
    const float gamma = a.state[so[2] + jj];
    float gw[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float gb = 0.0f, gg = 0.0f, gbe = 0.0f;
    for (int s = 0; s < 2; ++s) {
        const float *xh = a.xh0 + ((size_t)s * 3 * H + j) * B;
        const float *dy = a.da0 + ((size_t)s * 3 * H + j) * B;
        float pw[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, pb = 0.0f;
        const float2 r = bn_backward_column(
            xh, B, lane, gamma, a.inv0[s * 3 * H + j], [&](int i) { return dy[i]; },
            [&](int i, float v) {
                const float *x = gathered_row(a, s, i) + k0;
                for (int k = 0; k < K; ++k) pw[k] = fmaf(v, x[k], pw[k]);
                pb += v;
            });
        for (int k = 0; k < K; ++k) gw[k] += wave_sum(pw[k]);
        gb += wave_sum(pb);
        gbe += r.x;
        gg += r.y;
    }
    if (lane == 0) {
        for (int k = 0; k < K; ++k) a.grad[po[0] + jj * K + k] = gw[k];
        a.grad[po[1] + jj] = gb;
        a.grad[po[2] + jj] = gg;
        a.grad[po[3] + jj] = gbe;
    }
}

// The torch.optim.Adam step (adam_element, adam.h) of every trainable element, in place in the state; the step
// counts were advanced by this step's pmi_head_kernel
__global__ void pmi_adam_kernel(PmiTrainLayout L, float *state, float *m, float *v, const float *grad,
                                const int64_t *steps, const int *status, float lr)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= L.P || *status) return;
    int t = 0;
    while (t + 1 < kPmiTrainTensors && p >= L.poff[t + 1]) ++t;
    adam_element(state[L.soff[PmiTrainLayout::state_of(t)] + (p - L.poff[t])], m[p], v[p], grad[p], steps[t], lr);
}

__global__ void pmi_finalize_kernel(const int *status, int *errors, const float *acc, int64_t nb, float *avg_loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (*status) { *errors += 1; *avg_loss = NAN; return; }
    *avg_loss = *acc / (float)nb;
}

// The step kernels' arguments that do not change within a call; rows, the triples and n_uav are the caller's
StepArgs step_args(const PmiTrainDevice &d, const PmiTrainLaunch &q)
{
    StepArgs a;
    a.L = d.L; a.rows = q.rows; a.t_idx = q.t_idx; a.u_idx = q.u_idx; a.n_uav = q.n_uav; a.B = (int)q.batch;
    a.row0 = 0; a.step = 0;
    a.state = d.state; a.grad = d.grad; a.nbt = d.nbt; a.steps = d.opt.steps;
    a.xh0 = d.xh0; a.a0 = d.a0; a.da0 = d.da0; a.xh1 = d.xh1; a.a1 = d.a1; a.dz1 = d.dz1;
    a.inv0 = d.inv0; a.inv1 = d.inv1; a.go = d.go; a.acc = d.acc;
    a.losses = q.losses; a.outputs = q.outputs; a.status = d.opt.status;
    return a;
}

// Mini-batch steps [b0, b1) of a call, step b taking the triples from first + (b - b0) * B on
hipError_t launch_pmi_steps(const PmiTrainDevice &d, StepArgs a, int64_t b0, int64_t b1, int64_t first, hipStream_t st)
{
    const PmiTrainLayout &L = d.L;
    const int H = L.H, B = a.B;
    const dim3 blk(kWG);
    const dim3 g_branch((3 * H + kWavesPerWG - 1) / kWavesPerWG), g_fc1((H + kWavesPerWG - 1) / kWavesPerWG);
    const dim3 g_adam((L.P + kWG - 1) / kWG);
    const int K = 3 * H, N2 = 2 * B;
    auto tiles = [](int M, int N) { return dim3((unsigned)((N + kTN - 1) / kTN), (unsigned)((M + kTM - 1) / kTM)); };
    const float *W1 = d.state + L.soff[18];
    // operands in the feature-major scratch: (side, row) pairs n = s * B + i
    const Opnd none = {nullptr, 0, 0, 0, 0, 0, 0};
    // fc1 forward: z1(c, n) = sum_k W1[c][k] a0[s][k][i] + b1[c]  ->  xh1[s][c][i]
    const Opnd f_a = {W1, K, 1, 0, 0, 0, 0};
    const Opnd f_b = {d.a0, B, 1, 0, B, 0, (int64_t)K * B};
    const Opnd f_c = {d.xh1, B, 1, 0, B, 0, (int64_t)H * B};
    // fc1.weight gradient: g(c, k) = sum_n dz1[s][c][i] a0[s][k][i]
    const Opnd w_a = {d.dz1, B, 1, 0, B, 0, (int64_t)H * B};
    const Opnd w_b = {d.a0, 1, B, B, 0, (int64_t)K * B, 0};
    const Opnd w_c = {d.grad + L.poff[12], K, 1, 0, 0, 0, 0};
    // dL/d(branch output): da0(k, n) = sum_c W1[c][k] dz1[s][c][i], masked by the branch ReLU
    const Opnd x_a = {W1, 1, K, 0, 0, 0, 0};
    const Opnd x_b = {d.dz1, B, 1, 0, B, 0, (int64_t)H * B};
    const Opnd x_c = {d.da0, B, 1, 0, B, 0, (int64_t)K * B};
    const Opnd x_m = {d.a0, B, 1, 0, B, 0, (int64_t)K * B};
    for (int64_t b = b0; b < b1; ++b) {
        a.row0 = first + (b - b0) * B;
        a.step = (int)b;
        hipLaunchKernelGGL(pmi_branch_fwd_kernel, g_branch, blk, 0, st, a);
        hipLaunchKernelGGL(pmi_gemm_kernel, tiles(H, N2), blk, 0, st, f_a, f_b, f_c, H, N2, K, (int)kAddBias,
                           d.state + L.soff[19], none, d.opt.status);
        hipLaunchKernelGGL(pmi_bn1_fwd_kernel, g_fc1, blk, 0, st, a);
        hipLaunchKernelGGL(pmi_head_kernel, dim3(1), dim3(kHeadThreads), 0, st, a);
        hipLaunchKernelGGL(pmi_bn1_bwd_kernel, g_fc1, blk, 0, st, a);
        hipLaunchKernelGGL(pmi_gemm_kernel, tiles(H, K), blk, 0, st, w_a, w_b, w_c, H, K, N2, (int)kStore, nullptr,
                           none, d.opt.status);
        hipLaunchKernelGGL(pmi_gemm_kernel, tiles(K, N2), blk, 0, st, x_a, x_b, x_c, K, N2, H, (int)kReluMask, nullptr,
                           x_m, d.opt.status);
        hipLaunchKernelGGL(pmi_branch_bwd_kernel, g_branch, blk, 0, st, a);
        hipLaunchKernelGGL(pmi_adam_kernel, g_adam, blk, 0, st, L, d.state, d.opt.m, d.opt.v, d.grad, d.opt.steps,
                           d.opt.status, d.lr);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The gather of uavtrack_pmi_trainer_train_many and _select: draws [d0, d0 + n) of the triples, the two rows of draw
// d0 + j to dst[j][2][12].  One lane per (draw, side, V floats); the draw's source is found by a binary search over the
// table's group prefix, and a draw whose group lies outside the table's span [base[0], base[count]) is skipped (its
// rows of dst stay as they were).  Row offsets are 64-bit.  The call's verdict (pmi_begin_kernel, which has tested every
// triple against the whole timeline) is read first: a refused call loads nothing through its indices and stores nothing.
struct SelectArgs {
    PmiSourceTable src;
    const int64_t *t_idx, *u_idx;
    int64_t n_uav, d0, n;
    float *dst;
    int64_t *id_t, *id_u;                // nullable: identity triples (t' = j, u' = (0, 1)) that address dst as a history
    const int *status;
    int *errors;                         // nullable: the refusal count, for a call that ends with this kernel
};

template <int V>
__global__ void __launch_bounds__(kWG) pmi_select_kernel(SelectArgs a)
{
    constexpr int kPerRow = 12 / V, kPerDraw = 2 * kPerRow;
    const int64_t gid = (int64_t)blockIdx.x * kWG + threadIdx.x;
    if (*a.status) {
        if (gid == 0 && a.errors) *a.errors += 1;
        return;
    }
    const int64_t j = gid / kPerDraw;
    if (j >= a.n) return;
    const int r = (int)(gid - j * kPerDraw), side = r / kPerRow, c = r - side * kPerRow;
    if (r == 0 && a.id_t) {
        a.id_t[j] = j;
        a.id_u[2 * j] = 0;
        a.id_u[2 * j + 1] = 1;
    }
    const int64_t g = a.d0 + j, t = a.t_idx[g];
    if (t < a.src.base[0] || t >= a.src.base[a.src.count]) return;
    int lo = 0, hi = a.src.count;        // base[lo] <= t < base[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t >= a.src.base[mid]) lo = mid; else hi = mid;
    }
    const float *from = a.src.rows[lo] + ((t - a.src.base[lo]) * a.n_uav + a.u_idx[2 * g + side]) * 12 + c * V;
    float *to = a.dst + (j * 2 + side) * 12 + c * V;
    if (V == 4) *reinterpret_cast<float4 *>(to) = *reinterpret_cast<const float4 *>(from);
    else *to = *from;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

void launch_select(SelectArgs a, hipStream_t st)
{
    bool vec = aligned16(a.dst);
    for (int k = 0; k < a.src.count; ++k) vec = vec && aligned16(a.src.rows[k]);
    const int64_t lanes = a.n * (vec ? 6 : 24);
    const dim3 grid((unsigned)((lanes + kWG - 1) / kWG));
    if (vec) hipLaunchKernelGGL(pmi_select_kernel<4>, grid, dim3(kWG), 0, st, a);
    else hipLaunchKernelGGL(pmi_select_kernel<1>, grid, dim3(kWG), 0, st, a);
}

}  // namespace

hipError_t launch_pmi_train(const PmiTrainDevice &d, const PmiTrainLaunch &q, hipStream_t st)
{
    const int64_t nb = q.b2 / q.batch;
    hipLaunchKernelGGL(pmi_begin_kernel, dim3(1), dim3(kWG), 0, st, q.t_idx, q.u_idx, q.b2, q.n_rows / q.n_uav, q.n_uav,
                       d.opt.status, d.acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if ((e = launch_pmi_steps(d, step_args(d, q), 0, nb, 0, st)) != hipSuccess) return e;
    hipLaunchKernelGGL(pmi_finalize_kernel, dim3(1), dim3(64), 0, st, d.opt.status, d.opt.errors, d.acc, nb, q.avg_loss);
    return hipGetLastError();
}

// launch_pmi_train with the rows of each mini-batch gathered from the source list first: the scratch holds the rows of
// max_b draws, so the steps run in fills of max_b / batch mini-batches (one fill while b2 <= max_b), each a select
// launch and then the unchanged step kernels on the scratch through identity triples.  The range check stays
// pmi_begin_kernel's, on the caller's triples against the whole timeline.
hipError_t launch_pmi_train_many(const PmiTrainDevice &d, const PmiSourceTable &src, const PmiTrainLaunch &q,
                                 hipStream_t st)
{
    const int64_t nb = q.b2 / q.batch, per_fill = d.max_b / q.batch;
    hipLaunchKernelGGL(pmi_begin_kernel, dim3(1), dim3(kWG), 0, st, q.t_idx, q.u_idx, q.b2, q.n_rows / q.n_uav, q.n_uav,
                       d.opt.status, d.acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    StepArgs a = step_args(d, q);
    a.rows = d.sel; a.t_idx = d.sel_t; a.u_idx = d.sel_u; a.n_uav = 2;
    SelectArgs s;
    s.src = src; s.t_idx = q.t_idx; s.u_idx = q.u_idx; s.n_uav = q.n_uav;
    s.dst = d.sel; s.id_t = d.sel_t; s.id_u = d.sel_u; s.status = d.opt.status; s.errors = nullptr;
    for (int64_t b0 = 0; b0 < nb; b0 += per_fill) {
        const int64_t b1 = b0 + per_fill < nb ? b0 + per_fill : nb;
        s.d0 = b0 * q.batch;
        s.n = (b1 - b0) * q.batch;
        launch_select(s, st);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = launch_pmi_steps(d, a, b0, b1, 0, st)) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(pmi_finalize_kernel, dim3(1), dim3(64), 0, st, d.opt.status, d.opt.errors, d.acc, nb, q.avg_loss);
    return hipGetLastError();
}

hipError_t launch_pmi_select(const PmiTrainDevice &d, const PmiSourceTable &src, int64_t total_groups, int64_t n_uav,
                             const int64_t *t_idx, const int64_t *u_idx, int64_t b2, float *selected, hipStream_t st)
{
    hipLaunchKernelGGL(pmi_begin_kernel, dim3(1), dim3(kWG), 0, st, t_idx, u_idx, b2, total_groups, n_uav, d.opt.status,
                       d.acc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    SelectArgs s;
    s.src = src; s.t_idx = t_idx; s.u_idx = u_idx; s.n_uav = n_uav; s.d0 = 0; s.n = b2;
    s.dst = selected; s.id_t = nullptr; s.id_u = nullptr; s.status = d.opt.status; s.errors = d.opt.errors;
    launch_select(s, st);
    return hipGetLastError();
}

}  // namespace uavtrack

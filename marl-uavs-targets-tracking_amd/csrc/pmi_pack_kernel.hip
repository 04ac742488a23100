// pmi_pack_kernel.hip -- fold_pmi_state_dict (uavtrack/pmi.py) and the host side of uavtrack_set_pmi_weights restated
// on the device, for uavtrack_publish_pmi_weights and uavtrack_pmi_trainer_publish: the MAAC-R scorer's whole weights
// allocation written straight from the 26 fp32 device tensors of a PMINetwork in torch layouts, stream-ordered, with no
// allocation and no synchronisation, bitwise identical to the host path on the same numbers.  Three launches:
//   pmi_pack_fold_kernel     one thread per float of the folded network in the ABI layout at the padded width:
//                            scale = gamma / sqrt(var + 1e-5), W' = W scale (transposed to input-major),
//                            b' = (b - mean) scale + beta in fp64, each rounded once to fp32 -- numpy's operations in
//                            numpy's order -- zeros in the padding units, into the handle's scratch;
//   pmi_pack_bounds_kernel   one workgroup: per unit |b| + the sequential sum over k of |w_uk| xb[k] (one thread per
//                            unit and branch, the host's order), the maxima (free of order; they drop NaN as
//                            std::fmax), then the block scales S1 and T, the range-watch limits and the f16 verdict
//                            (pmi_pack.h: the host's own functions) into the scalar block;
//   pmi_pack_layout_kernel   one thread per 16-byte word of the four layouts (pack_pmi_blob, pack_pmi_x6, pack_pmi_l1,
//                            pack_pmi_t3: the index and split functions of pmi_pack.h), vector stores.
// Every word of the allocation is written on every call, whatever the verdict, so nothing of earlier weights survives.
// -ffp-contract=off (Makefile) keeps each product and sum rounded on its own, as on the host.

#include "pmi_pack.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kPackThreads = 1024;       // the bounds kernel's one workgroup: 16 wavefronts
constexpr int kFoldThreads = 256;

// tensor t of block b (PmiTrainLayout order): 0 weight [H][in], 1 bias, 2 bn weight, 3 bn bias, 4 running_mean, 5 running_var
__device__ __forceinline__ const float *block_tensor(const PmiPackArgs &a, int b, int t) { return a.t[b * 6 + t]; }

__device__ __forceinline__ double bn_scale(const PmiPackArgs &a, int b, int u)
{
    return (double)block_tensor(a, b, 2)[u] / sqrt((double)block_tensor(a, b, 5)[u] + 1e-5);
}
__device__ __forceinline__ float fold_weight(const PmiPackArgs &a, int b, int in, int k, int u)
{
    return (float)((double)block_tensor(a, b, 0)[(size_t)u * in + k] * bn_scale(a, b, u));
}
__device__ __forceinline__ float fold_bias(const PmiPackArgs &a, int b, int u)
{
    const double d = (double)block_tensor(a, b, 1)[u] - (double)block_tensor(a, b, 4)[u];
    return (float)(d * bn_scale(a, b, u) + (double)block_tensor(a, b, 3)[u]);
}

// the ABI layout at width HP: Wc[5][HP] bc[HP] Wo[4][HP] bo[HP] Wb[3][HP] bb[HP] W1[3 HP][HP] b1[HP] w2[HP] b2
__global__ __launch_bounds__(kFoldThreads) void pmi_pack_fold_kernel(PmiPackArgs a)
{
    const int H = a.H, HP = a.HP;
    const size_t head = (size_t)15 * HP, w1_len = (size_t)3 * HP * HP, n = head + w1_len + 2 * (size_t)HP + 1;
    for (size_t i = (size_t)blockIdx.x * kFoldThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kFoldThreads) {
        float v = 0.0f;
        if (i < head) {
            const int row = (int)(i / HP), u = (int)(i % HP);
            const int b = row < 6 ? 0 : (row < 11 ? 1 : 2), r0 = b == 0 ? 0 : (b == 1 ? 6 : 11), fan = 5 - b;
            if (u < H) v = row - r0 < fan ? fold_weight(a, b, fan, row - r0, u) : fold_bias(a, b, u);
        } else if (i < head + w1_len) {
            const size_t j = i - head;
            const int row = (int)(j / HP), u = (int)(j % HP), br = row / HP, kk = row % HP;
            if (u < H && kk < H) v = fold_weight(a, 3, 3 * H, br * H + kk, u);
        } else if (i < head + w1_len + HP) {
            const int u = (int)(i - head - w1_len);
            if (u < H) v = fold_bias(a, 3, u);
        } else if (i < head + w1_len + 2 * (size_t)HP) {
            const int u = (int)(i - head - w1_len - HP);
            if (u < H) v = a.t[24][u];
        } else {
            v = a.t[25][0];
        }
        a.fold[i] = v;
    }
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    return v;
}

__global__ __launch_bounds__(kPackThreads) void pmi_pack_bounds_kernel(PmiPackArgs a)
{
    constexpr int NV = 9;            // act_max, gain[3], bias[3], w1_max, the branch layers' largest |w|
    __shared__ double red[NV][kPackThreads / 64];
    const PmiBlobLayout L = PmiBlobLayout::make(a.HP);
    float *scal = a.blob + L.scal_off;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, HP = a.HP;
    if (L.t3_len == 0) {             // widths of the fp32 scorer alone: no planes, no scales, no verdict
        if (tid < kPmiScalWords) {
            float v = 0.0f;
            if (tid == kPmiScalScale || tid == kPmiScalInvScale || tid == kPmiScalS1 || tid == kPmiScalT) v = 1.0f;
            scal[tid] = v;
        }
        return;
    }
    double m[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) m[k] = 0.0;
    const int fan[3] = {5, 4, 3}, row0[3] = {0, 6, 11}, k0[3] = {0, 5, 9};
    for (int i = tid; i < 3 * HP; i += kPackThreads) {
        const int br = i / HP, u = i % HP;
        const float *pw = a.fold + (size_t)row0[br] * HP;
        double s = fabs((double)pw[(size_t)fan[br] * HP + u]), gsum = 0.0;
        const double bias = s;
        for (int k = 0; k < fan[br]; ++k) {
            const double w = fabs((double)pw[(size_t)k * HP + u]);
            s += w * a.xb[k0[br] + k];
            gsum += w;
        }
        m[0] = fmax(m[0], s);
#pragma unroll
        for (int b = 0; b < 3; ++b)
            if (b == br) { m[1 + b] = fmax(m[1 + b], gsum); m[4 + b] = fmax(m[4 + b], bias); }
    }
    const float *w1 = a.fold + (size_t)15 * HP;
    for (size_t i = tid; i < (size_t)3 * HP * HP; i += kPackThreads) m[7] = fmax(m[7], fabs((double)w1[i]));
    for (int i = tid; i < 15 * HP; i += kPackThreads) m[8] = fmax(m[8], fabs((double)a.fold[i]));
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        m[k] = wave_max(m[k]);
        if (lane == 0) red[k][wave] = m[k];
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int k = 0; k < NV; ++k)
            for (int w = 1; w < kPackThreads / 64; ++w) m[k] = fmax(m[k], red[k][w]);
        const double act_max = m[0], w1_max = m[7];
        const double w_max = fmax(fmax(w1_max, m[8]), a.pos2);
        const float s1 = pmi_scale_for(act_max, 512.0), tw = pmi_scale_for(w1_max, 32000.0);
        const float scale = s1 * tw;
        scal[kPmiScalScale] = scale;
        scal[kPmiScalInvScale] = 1.0f / scale;
        for (int br = 0; br < 3; ++br) scal[kPmiScalRng + br] = pmi_rng_inv(m[1 + br], m[4 + br], s1);
        scal[kPmiScalFit] = pmi_float(pmi_f16_fit(act_max, w_max) ? 1u : 0u);
        scal[kPmiScalS1] = s1;
        scal[kPmiScalT] = tw;
    }
}

__device__ __forceinline__ uint4 pack8(const uint16_t (&v)[8])
{
    return make_uint4(v[0] | ((uint32_t)v[1] << 16), v[2] | ((uint32_t)v[3] << 16), v[4] | ((uint32_t)v[5] << 16),
                      v[6] | ((uint32_t)v[7] << 16));
}

// Items, in this order: the 16-byte words of the fp32 blob's head (branch layers: a copy), of its fc1 block
// (pack_pmi_blob's lane order), of its tail up to the next piece (b1, w2, b2, zero padding); then per (w, s, l) the
// three x6 words and the two t3 words, and per (w, branch, l) the three l1 words.
__global__ __launch_bounds__(256) void pmi_pack_layout_kernel(PmiPackArgs a)
{
    const int HP = a.HP, NW = HP / 32, KH = 3 * HP / 2, KS = 3 * HP / 16;
    const PmiBlobLayout L = PmiBlobLayout::make(HP);
    const float *src = a.fold;
    const float *W1 = src + (size_t)15 * HP;
    const size_t n_head = (size_t)15 * HP / 4, n_w1 = (size_t)NW * (KH / 4) * 64;
    const size_t tail0 = (size_t)15 * HP + (size_t)3 * HP * HP, n_tail = (L.x6_off - tail0) / 4;
    const size_t n_fc1 = L.t3_len ? (size_t)NW * KS * 64 : 0, n_l1 = L.t3_len ? (size_t)NW * 3 * 64 : 0;
    const size_t total = n_head + n_w1 + n_tail + 2 * n_fc1 + n_l1;
    const float S1 = a.blob[L.scal_off + kPmiScalS1], T = a.blob[L.scal_off + kPmiScalT];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        size_t k = i;
        if (k < n_head) {
            reinterpret_cast<float4 *>(a.blob)[k] = reinterpret_cast<const float4 *>(src)[k];
            continue;
        }
        k -= n_head;
        if (k < n_w1) {
            const int l = (int)(k & 63), t4 = (int)((k >> 6) % (KH / 4)), w = (int)((k >> 6) / (KH / 4));
            const int col = w * 32 + (l & 31);
            float4 v;
            v.x = W1[(size_t)pmi_blob_row(t4, l, 0) * HP + col];
            v.y = W1[(size_t)pmi_blob_row(t4, l, 1) * HP + col];
            v.z = W1[(size_t)pmi_blob_row(t4, l, 2) * HP + col];
            v.w = W1[(size_t)pmi_blob_row(t4, l, 3) * HP + col];
            reinterpret_cast<float4 *>(a.blob + (size_t)15 * HP)[k] = v;
            continue;
        }
        k -= n_w1;
        if (k < n_tail) {
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const size_t e = tail0 + 4 * k + q;
                v[q] = e < L.n_dev ? src[e] : 0.0f;
            }
            reinterpret_cast<float4 *>(a.blob + tail0)[k] = make_float4(v[0], v[1], v[2], v[3]);
            continue;
        }
        k -= n_tail;
        if (k < 2 * n_fc1) {
            const bool t3 = k >= n_fc1;
            if (t3) k -= n_fc1;
            const int l = (int)(k & 63), s = (int)((k >> 6) % KS), w = (int)((k >> 6) / KS);
            const int col = w * 32 + (l & 31);
            uint16_t p0[8], p1[8], p2[8];
            if (!t3) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    uint16_t o[3];
                    pmi_split_x6(W1[(size_t)pmi_x6_row(s, l, j) * HP + col], o);
                    p0[j] = o[0]; p1[j] = o[1]; p2[j] = o[2];
                }
                uint4 *dst = reinterpret_cast<uint4 *>(a.blob + L.x6_off);
                dst[(((size_t)w * 3 + 0) * KS + s) * 64 + l] = pack8(p0);
                dst[(((size_t)w * 3 + 1) * KS + s) * 64 + l] = pack8(p1);
                dst[(((size_t)w * 3 + 2) * KS + s) * 64 + l] = pack8(p2);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) pmi_split_t3(W1[(size_t)pmi_t3_row(s, l, j) * HP + col], T, p0[j], p1[j]);
                uint4 *dst = reinterpret_cast<uint4 *>(a.blob + L.t3_off);
                dst[(((size_t)w * 2 + 0) * KS + s) * 64 + l] = pack8(p0);
                dst[(((size_t)w * 2 + 1) * KS + s) * 64 + l] = pack8(p1);
            }
            continue;
        }
        k -= 2 * n_fc1;
        {
            const int l = (int)(k & 63), j = (int)((k >> 6) % 3), w = (int)((k >> 6) / 3);
            uint16_t p0[8], p1[8], p2[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) pmi_split_l1(pmi_l1_value(src, HP, w, j, l, jj), S1, p0[jj], p1[jj], p2[jj]);
            uint4 *dst = reinterpret_cast<uint4 *>(a.blob + L.l1_off);
            dst[(((size_t)w * 3 + j) * 3 + 0) * 64 + l] = pack8(p0);
            dst[(((size_t)w * 3 + j) * 3 + 1) * 64 + l] = pack8(p1);
            dst[(((size_t)w * 3 + j) * 3 + 2) * 64 + l] = pack8(p2);
        }
    }
}

}  // namespace

hipError_t launch_pmi_pack(const PmiPackArgs &a, hipStream_t st)
{
    const PmiBlobLayout L = PmiBlobLayout::make(a.HP);
    const unsigned fold_groups = (unsigned)((L.n_dev + kFoldThreads - 1) / kFoldThreads);
    hipLaunchKernelGGL(pmi_pack_fold_kernel, dim3(fold_groups), dim3(kFoldThreads), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(pmi_pack_bounds_kernel, dim3(1), dim3(kPackThreads), 0, st, a);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const size_t words = (L.scal_off + 3) / 4;       // an upper bound of the layout kernel's items
    hipLaunchKernelGGL(pmi_pack_layout_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace uavtrack

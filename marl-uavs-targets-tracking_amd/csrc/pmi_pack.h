// pmi_pack.h -- the one statement of everything the MAAC-R scorer's weight allocation is made of: where each piece lies
// (PmiBlobLayout), which element of the folded network lands in which word of the four packed layouts, how a value is
// split into bf16 / f16 planes, and how the block scales, the range-watch limits and the f16 verdict follow from the
// bounds.  The host packers (pmi_kernel.hip, uavtrack_set_pmi_weights) and the device pack (pmi_pack_kernel.hip,
// uavtrack_publish_pmi_weights) both go through these functions, so the two cannot round apart.  Every operation is an
// IEEE basic operation on both sides (-ffp-contract=off, Makefile); a NaN that a split produces or passes on is written
// as the canonical quiet NaN, because the sign and payload of a generated NaN are the one thing the two processors do
// not agree on.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "pmi_net.h"
#include "uavtrack.h"

namespace uavtrack {

constexpr int kPmiX6MaxHidden = 128;                // widest layer whose three bf16 planes stay register-resident (4 waves, one per SIMD)
constexpr int kPmiX6MinHidden = 64;                 // (narrower layers have fewer k-steps than the producer has pairs to hide)

// The weights allocation, in floats: the fp32 blob in scorer order (pack_pmi_blob), padded to 16 bytes; for the widths
// with split kernels (64 / 96 / 128) the bf16 planes of fc1 (pack_pmi_x6), the f16 planes of the branch layers
// (pack_pmi_l1) and of fc1 (pack_pmi_t3); then the scalar block every width has.
struct PmiBlobLayout {
    size_t n_dev, x6_off, x6_len, l1_off, l1_len, t3_off, t3_len, scal_off, total;
    __host__ __device__ static PmiBlobLayout make(int hp)
    {
        PmiBlobLayout L;
        const size_t HP = (size_t)hp;
        const bool split = hp >= kPmiX6MinHidden && hp <= kPmiX6MaxHidden;
        L.n_dev = 12 * HP + 3 * HP + 3 * HP * HP + HP + HP + 1;
        L.x6_off = (L.n_dev + 3) & ~(size_t)3;
        L.x6_len = split ? 3 * HP * HP * 3 / 2 : 0;                 // 3 planes x 2 B
        L.l1_off = L.x6_off + L.x6_len;
        L.l1_len = split ? (HP / 32) * 3 * 3 * 64 * 8 / 2 : 0;      // [w][branch][3 planes][lane][8] x 2 B
        L.t3_off = L.l1_off + L.l1_len;
        L.t3_len = split ? 3 * HP * HP : 0;                         // 2 planes x 2 B
        L.scal_off = L.t3_off + L.t3_len;
        L.total = L.scal_off + 8;
        return L;
    }
};

// The scalar block (8 words at scal_off): what pmi_score_t3_kernel needs beside the planes and what only the weights
// decide.  It lives in device memory because a device publish changes it without the host knowing, and because a
// captured graph would bake kernel arguments in.
enum {
    kPmiScalScale = 0,       // S1 * T: the power of two the t3 kernel's layer-2 accumulators carry
    kPmiScalInvScale = 1,    // its reciprocal
    kPmiScalRng = 2,         // [3] 1 / the largest |x| each branch's inputs may reach (the run-time range watch)
    kPmiScalFit = 5,         // uint32: 1 if weights and activation bounds fit f16's range (the t3 planes may be used)
    kPmiScalS1 = 6,          // S1 and T on their own (the pack kernels read them back; inspection)
    kPmiScalT = 7,
    kPmiScalWords = 8
};

__host__ __device__ inline uint32_t pmi_bits(float v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }
__host__ __device__ inline float pmi_float(uint32_t u) { float v; __builtin_memcpy(&v, &u, 4); return v; }
__host__ __device__ inline float pmi_canon(float v) { return v != v ? pmi_float(0x7FC00000u) : v; }
// A product that is rounded to fp32 on its own before anything else happens to it.  The device compiler otherwise folds a
// multiplication and the conversion to f16 behind it into one mixed-precision FMA with a +0 addend, which turns a product of
// -0 into +0 (and rounds once instead of twice); the host has no such instruction.
__host__ __device__ inline float pmi_rounded(float v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(v));
#endif
    return v;
}
// f16 (round to nearest even) of a float, as bits
__host__ __device__ inline uint16_t pmi_f16_bits(float v)
{
    if (v != v) return 0x7E00u;
    const _Float16 h = (_Float16)v;
    uint16_t b;
    __builtin_memcpy(&b, &h, 2);
    return b;
}

// x = hi + mid + lo by truncation to bf16 (exact: each remainder has at most 16 significant bits left)
__host__ __device__ inline void pmi_split_x6(float v, uint16_t out[3])
{
    for (int p = 0; p < 3; ++p) {
        v = pmi_canon(v);
        const uint32_t u = pmi_bits(v) & 0xFFFF0000u;
        out[p] = (uint16_t)(u >> 16);
        v -= pmi_float(u);
    }
}
// fc1 block-scaled for pmi_score_t3_kernel: f16(T w) and f16(T w - plane 0), T a power of two
__host__ __device__ inline void pmi_split_t3(float w, float T, uint16_t &hi, uint16_t &lo)
{
    const float v = pmi_rounded(T * w);
    const _Float16 h = (_Float16)v;
    hi = pmi_f16_bits(v);
    lo = pmi_f16_bits(pmi_rounded(v - (float)h));
}
// a branch-layer weight block-scaled by S1: f16(v), f16(v - plane 0), plane 0 * 2^-11
__host__ __device__ inline void pmi_split_l1(float w, float S1, uint16_t &hi, uint16_t &lo, uint16_t &hs)
{
    const float v = pmi_rounded(w * S1);
    const _Float16 h = (_Float16)v;
    hi = pmi_f16_bits(v);
    lo = pmi_f16_bits(pmi_rounded(v - (float)h));
    hs = pmi_f16_bits(pmi_rounded((float)h * (1.0f / 2048.0f)));
}

// ---- which element of the folded, padded blob (the ABI layout at width H = the padded width) each packed word holds
// pack_pmi_blob: element q of lane l, k-step group t4: W1 row, the column being 32 w + (l & 31)
__host__ __device__ inline int pmi_blob_row(int t4, int l, int q) { return 2 * (4 * t4 + q) + (l >> 5); }
// pack_pmi_x6: value j of lane l, k-step s
__host__ __device__ inline int pmi_x6_row(int s, int l, int j) { return 16 * s + 8 * (l >> 5) + j; }
// pack_pmi_t3: k-position -> fc1 input: inside a block of 32, position q = 16 kh + r holds unit (r & 3) + 8 (r >> 2) + 4 kh,
// the order in which pmi_score_t3_kernel's lanes store their activations
__host__ __device__ inline int pmi_t3_row(int s, int l, int j)
{
    const int kp = 16 * s + 8 * (l >> 5) + j, q = kp & 31, r = q & 15;
    return (kp & ~31) + (r & 3) + 8 * (r >> 2) + 4 * (q >> 4);
}
// pack_pmi_l1: value jj of lane l in the block of wavefront w and branch j: unit 32 w + (l & 31) against "input"
// k = 8 (l >> 5) + jj of x_0..x_11, 1, 0, 0, 0 -- the branch's own inputs carry its weights, input 12 its bias
__host__ __device__ inline float pmi_l1_value(const float *blob, int H, int w, int j, int l, int jj)
{
    const int k0[3] = {0, 5, 9}, fan[3] = {5, 4, 3}, woff[3] = {0, 6, 11};
    const int unit = 32 * w + (l & 31), k = 8 * (l >> 5) + jj;
    if (k >= k0[j] && k < k0[j] + fan[j]) return blob[(size_t)(woff[j] + k - k0[j]) * H + unit];
    if (k == 12) return blob[(size_t)(woff[j] + fan[j]) * H + unit];
    return 0.0f;
}

// ---- bounds -> scales, limits, verdict
// 2^e, e = floor(log2(target / bound)) kept within [-6, 15]: the largest power of two that takes `bound` to at most
// `target`.  The floor comes from the quotient's exponent field, so it is exact and the same on every processor (a
// libm log2 rounds to the integer above for quotients a few ulps below a power of two).  No positive bound: 2^15.
__host__ __device__ inline float pmi_scale_for(double bound, double target)
{
    int e = 15;
    if (bound > 0.0) {
        const double r = target / bound;
        uint64_t b;
        __builtin_memcpy(&b, &r, 8);
        const int be = (int)((b >> 52) & 0x7FF);
        if (!(r > 0.0)) e = -6;                      // an infinite bound
        else if (be == 0x7FF) e = 15;
        else e = be == 0 ? -1023 : be - 1023;
    }
    e = e < -6 ? -6 : (e > 15 ? 15 : e);
    return pmi_float((uint32_t)(127 + e) << 23);
}
// The run-time watch of the f16 kernel: an activation of a branch stays below 60000 / S1 while
// |x| <= (60000 / S1 - max|b|) / max_u sum_k|w_uk| over the branch's inputs, and an input splits into normal f16 planes
// below 30000; the kernel compares the largest |x| of a tile with the smaller of the two.  Returns 1 / that limit.
__host__ __device__ inline float pmi_rng_inv(double gain, double bias, float s1)
{
    double lim = 30000.0;
    if (gain > 0.0) lim = fmin(lim, (60000.0 / (double)s1 - bias) / gain);
    return lim > 0.0 ? (float)(1.0 / lim) : __builtin_huge_valf();
}
// every MFMA operand of the f16 kernel inside half of f16's range
__host__ __device__ inline bool pmi_f16_fit(double act_max, double w_max)
{
    return act_max - act_max == 0.0 && act_max < 32000.0 && w_max < 32000.0;     // (x - x == 0: finite)
}

// pmi_pack_kernel.hip -- fold_pmi_state_dict + the host side of uavtrack_set_pmi_weights restated on the device
struct PmiPackArgs {
    const float *t[kPmiStateTensors];      // the network's 26 fp32 tensors, torch layouts, PmiTrainLayout order
    int H, HP;                             // hidden width, padded
    double xb[UAVTRACK_OBS_DIM];           // nominal bounds of the pair inputs |x_k| (pmi_input_bounds)
    double pos2;                           // ... the largest of them, an MFMA operand of the f16 kernel too
    float *fold;                           // scratch [n_dev]: the folded network in the ABI layout at width HP
    float *blob;                           // the weights allocation (PmiBlobLayout::make(HP))
};
hipError_t launch_pmi_pack(const PmiPackArgs &a, hipStream_t stream);

// pmi_kernel.hip -- the host packers of uavtrack_set_pmi_weights
void pack_pmi_blob(const float *abi_blob, float *device_order, int hidden);
void pack_pmi_x6(const float *abi_blob, uint16_t *planes, int hidden);
void pack_pmi_t3(const float *abi_blob, uint16_t *planes, int hidden, float T);
void pack_pmi_l1(const float *abi_blob, uint16_t *planes, int hidden, float S1);

}  // namespace uavtrack

// replay_kernel.hip -- the reference's PrioritizedReplayBuffer (train.py:73-139) on the device: add (train.py:87-96)
// straight from a rollout's outputs, and sample (train.py:98-112) with replacement from P(i) = p_i^alpha / sum_j p_j^alpha.
//
// Sampling is a chain of stream-ordered launches, none of which synchronises or allocates:
//   replay_begin_kernel     one thread: this call's Philox counter (the device call counter, then advanced), status and
//                           the batch minimum of P cleared;
//   replay_tile_kernel      one workgroup per tile of kReplayTile slots: w_i = p_i^alpha in fp32 (the reference's
//                           float32 `priorities ** alpha`), their fp64 sum in a fixed order, the tile's last slot with
//                           w > 0, and a refusal bit for a NaN, infinite or negative priority;
//   replay_scan_kernel      one workgroup: the tile sums -> their inclusive fp64 prefix (the coarse CDF); an all-zero
//                           ring is refused here;
//   replay_draw_kernel      one wavefront per draw: u in [0, 1) from 53 Philox bits, x = u * total, the first tile whose
//                           prefix exceeds x (binary search), then the wavefront rescans that tile (32 slots per lane,
//                           a wave prefix sum of the lane sums, a serial search in the lane) for the first slot whose
//                           running sum exceeds x: searchsorted(cdf, x, side='right'), as np.random.choice;
//   replay_min_kernel,      (only when weights are asked for) (count * P(i))^-beta / max over the batch, the maximum
//   replay_weight_kernel    taken from the smallest P(i) of the batch (a workgroup reduction, then one order-independent
//                           atomic min per workgroup).  beta is the caller's, or (uavtrack_replay_sample_annealed) read
//                           off a linear schedule at this call's number, so a replayed graph anneals.
// The sums are fp64 in a fixed order, but not one order: the scans associate a prefix differently from its predecessor,
// so where the rescan and the coarse prefix disagree in the last bit, or a lane or tile holding no w > 0 gets a prefix
// an ulp above its predecessor's and x falls in between, the rule is: the draw takes the last slot with w > 0 at or
// before the lane (tile) it was sent to.  One exists: a prefix over nothing but zeros is exactly 0, and never exceeds
// x >= 0.  x >= total cannot happen: u <= 1 - 2^-53 and total >= 2^-149 is a normal double, so u * total rounds below
// total.  So a draw lands only on a slot in [0, count) with w > 0.  A refused call writes slot 0 and NaN weights.
//
// The uniform draw (the reference's ReplayBuffer.sample, train.py:56-58: random.sample, without replacement) is
// replay_begin_kernel and replay_uniform_kernel: one thread per draw, O(k) whatever the ring holds.  It reads nothing
// of the ring, so it has no refusal.  The sweep (on-policy epochs: every slot of a ring window once per epoch, a
// minibatch per call) is replay_cursor_kernel and replay_sweep_kernel: the same walk, keyed by the epoch and started at
// the call's place in it, both read off a cursor the caller owns; the handle's counter is not touched.
//
// Adding (launch_replay_add, one ReplayAdd request) is two reductions (the maximum of the whole priorities array,
// train.py:87-88; skipped for a ring without priorities, a uniform ring) and one write kernel over the request's ring
// window, the last min(n, capacity) transitions from ring.pos on:
//   replay_write_kernel        flat and rollout forms: each thread owns one source transition f, reads obs[f] once and
//                              writes it as the next state of f and the state of f + agents; <true> (done given) writes
//                              start_obs[f] as that state instead wherever the done flag of f's environment-step fired;
//   replay_write_nstep_kernel  the n-step form: a thread folds up to n rewards of its agent into the stored reward, takes
//                              the next state from the end of that window and leaves the window's discount in a fifth
//                              per-slot store;
//   replay_lambda_scan_kernel  the lambda form, behind replay_write_kernel and over the same window: one thread per agent
//                              chain walks the rollout backwards, carries the lambda-return G and overwrites the written
//                              slots' rewards with R_t, leaving d_t in the discount store;
//   replay_gae_scan_kernel     the GAE form: the same walk and the same fold, storing the lambda-return G_t itself as the
//                              reward, a discount of +0 and the advantage G_t - V(s_t) in a seventh per-slot store.

#include "replay.h"
#include "philox.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kSW = 256;                       // threads per workgroup of the tile and write kernels
constexpr int kPerThread = kReplayTile / kSW;  // slots per thread in the tile kernel
constexpr int kPerLane = kReplayTile / 64;     // slots per lane in the draw kernel's rescan
constexpr int kScanW = 1024;                   // threads of the scan kernel
static_assert(kReplayTile % kSW == 0 && kReplayTile % 64 == 0, "tile geometry");

// p^alpha of slot i as the reference's float32 array power; 0 beyond count.  bad: a NaN, infinite or negative priority.
__device__ __forceinline__ float slot_weight(const float *prio, int64_t i, int64_t count, float alpha, bool &bad)
{
    if (i >= count) return 0.0f;
    const float p = prio[i];
    if (!(p >= 0.0f) || isinf(p)) { bad = true; return 0.0f; }
    return alpha == 1.0f ? p : powf(p, alpha);
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_inclusive_scan(double v, int lane)
{
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// The last slot with w > 0 in tiles <= t, for a whole wavefront: the wave walks tile_last back from t, 64 tiles a step
// (-1 if there is none).  Past the first step only for a draw that rounding sent into a tile holding no w > 0.
__device__ __forceinline__ int64_t last_positive_upto(const int64_t *tile_last, int t, int lane)
{
    for (int top = t; top >= 0; top -= 64) {
        const int i = top - lane;
        const int64_t v = i >= 0 ? tile_last[i] : -1;
        const unsigned long long has = __ballot(v >= 0);
        if (has) return __shfl(v, __ffsll(has) - 1, 64);          // the lowest lane holds the highest tile
    }
    return -1;
}

// max that keeps a NaN once seen (torch.max propagates NaN)
__device__ __forceinline__ float nan_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ void replay_begin_kernel(uint64_t *counter, int *status, unsigned long long *pmin)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    counter[1] = counter[0];
    counter[0] += 1;
    *status = 0;
    *pmin = 0x7FF0000000000000ull;             // +inf
}

__global__ void __launch_bounds__(kSW) replay_tile_kernel(const float *prio, int64_t count, float alpha, double *tile_sum,
                                                          int64_t *tile_last, int *status)
{
    __shared__ double wsum[kSW / 64];
    __shared__ unsigned long long last;        // 1 + the last slot with w > 0 (0: none)
    __shared__ int bad_any;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) { last = 0; bad_any = 0; }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kReplayTile + (int64_t)tid * kPerThread;
    bool bad = false;
    double s = 0.0;
    int64_t mylast = -1;
#pragma unroll
    for (int q = 0; q < kPerThread; ++q) {
        const float w = slot_weight(prio, base + q, count, alpha, bad);
        s += (double)w;
        if (w > 0.0f) mylast = base + q;
    }
    if (mylast >= 0) atomicMax(&last, (unsigned long long)(mylast + 1));
    if (bad) bad_any = 1;
    s = wave_sum(s);
    if (lane == 0) wsum[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < kSW / 64; ++w) t += wsum[w];
        tile_sum[blockIdx.x] = t;
        tile_last[blockIdx.x] = (int64_t)last - 1;
        if (bad_any) atomicOr(status, 1);
    }
}

// One workgroup: tile sums -> inclusive prefix in place.  Thread c owns a contiguous chunk of tiles.
__global__ void __launch_bounds__(kScanW) replay_scan_kernel(double *prefix, int ntiles, int *status, int *errors)
{
    __shared__ double wtot[kScanW / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chunk = (ntiles + kScanW - 1) / kScanW;
    const int b = tid * chunk, e = min(ntiles, b + chunk);
    double s = 0.0;
    for (int t = b; t < e; ++t) s += prefix[t];
    const double incl = wave_inclusive_scan(s, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    double off = 0.0;
    for (int w = 0; w < wave; ++w) off += wtot[w];
    double excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0.0;
    double run = off + excl;
    for (int t = b; t < e; ++t) { run += prefix[t]; prefix[t] = run; }
    __syncthreads();
    if (tid == 0) {
        const double total = prefix[ntiles - 1];
        int st = *status;
        if (!(total > 0.0)) st |= 2;
        *status = st;
        if (st) *errors += 1;
    }
}

struct DrawArgs {
    const float *prio;
    const double *prefix;
    const int64_t *tile_last;
    const uint64_t *counter;
    const int *status;
    double *pdraw;
    int64_t *indices;
    int64_t count, k;
    int ntiles;
    float alpha;
    uint32_t k0, k1;
};

__global__ void __launch_bounds__(kSW) replay_draw_kernel(DrawArgs a)
{
    const int lane = threadIdx.x & 63;
    const int64_t j = (int64_t)blockIdx.x * (kSW / 64) + (threadIdx.x >> 6);
    if (j >= a.k) return;                      // (whole wavefronts)
    if (*a.status) {
        if (lane == 0) { a.indices[j] = 0; a.pdraw[j] = NAN; }
        return;
    }
    const uint64_t call = a.counter[1];
    const Philox4 r = philox4x32_10((uint32_t)j, (uint32_t)call, (uint32_t)(call >> 32), kReplayDomain, a.k0, a.k1);
    const uint64_t bits = ((uint64_t)r.v[0] << 21) | (uint64_t)(r.v[1] >> 11);
    const double u = (double)bits * 0x1p-53;
    const double total = a.prefix[a.ntiles - 1];
    const double x = u * total;

    // the first tile whose inclusive prefix exceeds x
    int lo = 0, hi = a.ntiles;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a.prefix[mid] > x) hi = mid; else lo = mid + 1;
    }
    int64_t slot;
    if (lo == a.ntiles) {
        slot = last_positive_upto(a.tile_last, a.ntiles - 1, lane);   // x >= total: unreachable (see the top)
    } else {
        const int t = lo;
        const double rem = x - (t > 0 ? a.prefix[t - 1] : 0.0);     // >= 0: prefix[t - 1] <= x
        const int64_t base = (int64_t)t * kReplayTile + (int64_t)lane * kPerLane;
        bool bad = false;
        double s = 0.0;
        for (int q = 0; q < kPerLane; ++q) s += (double)slot_weight(a.prio, base + q, a.count, a.alpha, bad);
        const unsigned long long nzl = __ballot(s > 0.0);             // the lanes holding a w > 0
        const double incl = wave_inclusive_scan(s, lane);
        double excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = 0.0;
        const unsigned long long hit = __ballot(incl > rem);
        if (hit == 0) {
            // the rescan's total fell short of the tile sum in the last bit (the tile's last slot with w > 0), or
            // tile t holds no w > 0 (its prefix rounded an ulp above its predecessor's): the last slot with w > 0
            // before it.  There is one: a prefix over nothing but zero tiles is exactly 0 <= x.
            slot = a.tile_last[t];
            if (slot < 0) slot = last_positive_upto(a.tile_last, t - 1, lane);
        } else {
            const int L = __ffsll(hit) - 1;
            int64_t mine = -1;
            if (lane == L) {
                const double want = rem - excl;
                double c = 0.0;
                int64_t lastnz = -1;
                for (int q = 0; q < kPerLane && mine < 0; ++q) {      // the same weights, summed in the same order
                    const float w = slot_weight(a.prio, base + q, a.count, a.alpha, bad);
                    if (w > 0.0f) lastnz = base + q;
                    c += (double)w;
                    if (c > want) mine = base + q;
                }
                if (mine < 0) mine = lastnz;    // (rem - excl) rounded past the lane's own sum
            }
            slot = __shfl(mine, L, 64);
            if (slot < 0) {
                // lane L holds no w > 0 (its scan rounded an ulp above its predecessor's): the last slot with w > 0 of
                // the lanes before it.  There is one: lanes 0..L all zero would scan to exactly 0 <= rem.
                const unsigned long long below = nzl & ((1ull << L) - 1);
                const int P = 63 - __clzll(below);
                int64_t pl = -1;
                if (lane == P)
                    for (int q = 0; q < kPerLane; ++q)
                        if (slot_weight(a.prio, base + q, a.count, a.alpha, bad) > 0.0f) pl = base + q;
                slot = __shfl(pl, P & 63, 64);
            }
        }
    }
    if (slot < 0 || slot >= a.count) slot = 0;  // unreachable (see the top); kept so no index ever leaves the ring
    if (lane == 0) {
        bool bad = false;
        const double p = (double)slot_weight(a.prio, slot, a.count, a.alpha, bad) / total;
        a.indices[j] = slot;
        a.pdraw[j] = p;
    }
}

// the batch minimum of P(i): one atomic min per workgroup (positive doubles order as their bits, so the result does not
// depend on the order of the atomics)
__global__ void __launch_bounds__(kSW) replay_min_kernel(const double *pdraw, int64_t k, unsigned long long *pmin)
{
    __shared__ double wm[kSW / 64];
    double m = INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kSW + threadIdx.x; i < k; i += (int64_t)gridDim.x * kSW) m = fmin(m, pdraw[i]);
    for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSW / 64; ++w) m = fmin(m, wm[w]);
        atomicMin(pmin, (unsigned long long)__double_as_longlong(m));
    }
}

// beta of call number c: beta0 + (beta1 - beta0) * min(1, c / anneal_calls), every operation rounded on its own (no
// fused multiply-add), so the host forms the same double from the same expression
__device__ __forceinline__ double annealed_beta(double beta0, double beta1, int64_t anneal_calls, uint64_t c)
{
#pragma clang fp contract(off)
    const double frac = fmin(1.0, (double)c / (double)anneal_calls);
    const double step = (beta1 - beta0) * frac;
    return beta0 + step;
}

__global__ void replay_weight_kernel(const double *pdraw, int64_t k, int64_t count, double beta0, double beta1,
                                     int64_t anneal_calls, const uint64_t *counter, const unsigned long long *pmin,
                                     const int *status, float *weights)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= k) return;
    if (*status) { weights[i] = NAN; return; }
    const double beta = anneal_calls > 0 ? annealed_beta(beta0, beta1, anneal_calls, counter[1]) : beta0;
    const double n = (double)count;
    const double wmax = pow(n * __longlong_as_double((long long)*pmin), -beta);
    weights[i] = (float)(pow(n * pdraw[i], -beta) / wmax);
}

// ---- the uniform draw: one thread per draw

// murmur3's 32-bit finaliser (Appleby, MurmurHash3, public domain)
__device__ __forceinline__ uint32_t fmix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x85EBCA6Bu;
    x ^= x >> 13; x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

// pi(x) walked below count: pi is a balanced Feistel network on 2 * half bits (count <= 4^half), round r's function
// fmix32(R + key_r) mod 2^half, the keys Philox blocks of (seed, number) in the stream DOMAIN names.  The walk stays on
// the cycle of pi through x < count, so it ends, and no two starts below count meet: pi is a bijection and each walk
// stops at the first value below count after its own start.  So the starts [0, count) map onto a permutation of
// [0, count).  What the uniform draw (number = the call) and the sweep (number = the epoch) share.
template <uint32_t DOMAIN>
__device__ __forceinline__ uint64_t keyed_walk(uint64_t x, uint64_t number, int64_t count, int half, uint32_t k0, uint32_t k1)
{
    uint32_t key[kUniformRounds];
#pragma unroll
    for (int i = 0; i < kUniformRounds / 4; ++i) {
        const Philox4 r = philox4x32_10((uint32_t)i, (uint32_t)number, (uint32_t)(number >> 32), DOMAIN, k0, k1);
#pragma unroll
        for (int w = 0; w < 4; ++w) key[4 * i + w] = r.v[w];
    }
    const uint32_t mask = (1u << half) - 1u;
    do {
        uint32_t L = (uint32_t)(x >> half), R = (uint32_t)x & mask;
#pragma unroll
        for (int r = 0; r < kUniformRounds; ++r) {
            const uint32_t t = L ^ (fmix32(R + key[r]) & mask);
            L = R;
            R = t;
        }
        x = ((uint64_t)L << half) | R;
    } while (x >= (uint64_t)count);
    return x;
}

// indices[j] = pi_call(j) walked below count
__global__ void __launch_bounds__(kSW) replay_uniform_kernel(const uint64_t *counter, int64_t count, int64_t k, int half,
                                                             uint32_t k0, uint32_t k1, int64_t *indices)
{
    const int64_t j = (int64_t)blockIdx.x * kSW + threadIdx.x;
    if (j >= k) return;
    indices[j] = (int64_t)keyed_walk<kUniformDomain>((uint64_t)j, counter[1], count, half, k0, k1);
}

// ---- the sweep: the whole of an epoch's permutation of a ring window, one minibatch of n per call

// the caller's cursor as replay_begin_kernel treats the handle's counter: this call's number, then advanced
__global__ void replay_cursor_kernel(uint64_t *cursor)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    cursor[1] = cursor[0];
    cursor[0] += 1;
}

struct SweepArgs {
    const uint64_t *cursor;
    int64_t *indices;
    int64_t first, length, n, cap;             // the window's first slot and its length W; n <= W <= cap, first < cap
    int half;
    uint32_t k0, k1;
};

// Call q = cursor[1] is minibatch m = q % M of epoch e = q / M, M = W / n: indices[j] = first + sigma_e(m n + j) wrapped
// at cap, sigma_e the walk keyed by (seed, e).  m n + j < M n <= W is a start inside the window; first + x < 2 cap, so
// one subtraction wraps.
__global__ void __launch_bounds__(kSW) replay_sweep_kernel(SweepArgs a)
{
    const int64_t j = (int64_t)blockIdx.x * kSW + threadIdx.x;
    if (j >= a.n) return;
    const uint64_t q = a.cursor[1], M = (uint64_t)(a.length / a.n);
    const uint64_t e = q / M, m = q - e * M;
    const uint64_t x = keyed_walk<kSweepDomain>(m * (uint64_t)a.n + (uint64_t)j, e, a.length, a.half, a.k0, a.k1);
    const int64_t slot = a.first + (int64_t)x;
    a.indices[j] = slot >= a.cap ? slot - a.cap : slot;
}

// ---- add

__global__ void __launch_bounds__(kSW) replay_max_kernel(const float *prio, int64_t capacity, float *parts)
{
    __shared__ float wm[kSW / 64];
    float m = -INFINITY;
    for (int64_t i = (int64_t)blockIdx.x * kSW + threadIdx.x; i < capacity; i += (int64_t)gridDim.x * kSW)
        m = nan_max(m, prio[i]);
    for (int o = 32; o > 0; o >>= 1) m = nan_max(m, __shfl_down(m, o, 64));
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kSW / 64; ++w) m = nan_max(m, wm[w]);
        parts[blockIdx.x] = m;
    }
}

// parts[kReplayMaxParts] = the maximum of parts[0, groups), or 1.0 for an empty ring (train.py:87-88)
__global__ void replay_top_kernel(float *parts, int groups, int empty)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float m = -INFINITY;
    for (int g = 0; g < groups; ++g) m = nan_max(m, parts[g]);
    parts[kReplayMaxParts] = empty ? 1.0f : m;
}

// The slots an add of n transitions writes: transitions [skip, n) into start, start + 1, ... (mod cap)
struct RingWindow {
    int64_t n, skip, start, cap;
};

RingWindow ring_window(const ReplayRingView &ring, int64_t n)
{
    RingWindow w;
    w.n = n; w.cap = ring.capacity;
    w.skip = n > w.cap ? n - w.cap : 0;
    w.start = (ring.pos + w.skip) % w.cap;
    return w;
}

// the slot of transition f in [skip, n): f - skip < cap and start < cap, so one subtraction wraps
__device__ __forceinline__ int64_t window_slot(const RingWindow &w, int64_t f)
{
    const int64_t slot = w.start + (f - w.skip);
    return slot >= w.cap ? slot - w.cap : slot;
}

// What every add kernel is given beside the ring: the source and the window.  n = steps * agents, agents = envs * n_uav.
// The order matters only to how the kernel arguments are fetched: what the lambda scan reads (skip .. done) is the tail,
// and its own arguments follow, so they stay the one span they were when the scan had a struct of its own.
struct AddSource {
    const float *obs_in;                       // rollout forms: [agents][12]; nullptr: the flat form
    const float *states, *next;                // flat: states [n][12]; flat: next states, rollout forms: obs [n][12]
    const int32_t *actions;                    // [n]
    const float *start_obs;                    // [n][12], read only where done fired
    const float *top;                          // the priority new transitions enter at
    RingWindow w;
    int64_t agents, envs, n_uav, steps;
    const float *rewards;                      // [n]
    const uint8_t *done;                       // nullable [steps][envs]
};

struct AddArgs {
    ReplayRingView ring;
    AddSource s;
};

__device__ __forceinline__ void copy_row(float *dst, const float *src)
{
    const float4 *s = reinterpret_cast<const float4 *>(src);
    float4 *d = reinterpret_cast<float4 *>(dst);
    const float4 a = s[0], b = s[1], c = s[2];
    d[0] = a; d[1] = b; d[2] = c;
}

template <bool EPISODES>
__global__ void __launch_bounds__(kSW) replay_write_kernel(AddArgs a)
{
    const AddSource &s = a.s;
    // what transition g + agents acted on: obs[g], or the fresh state's observation where g's episode ended at g
    auto state_after = [&](int64_t g, const float *obs_row) {
        if (EPISODES && s.done[g / s.n_uav]) return s.start_obs + g * 12;
        return obs_row;
    };
    const float top = a.ring.priorities ? *s.top : 0.0f;
    for (int64_t f = s.w.skip + (int64_t)blockIdx.x * kSW + threadIdx.x; f < s.w.n; f += (int64_t)gridDim.x * kSW) {
        const int64_t slot = window_slot(s.w, f);
        const float *row = s.next + f * 12;
        copy_row(a.ring.next_states + slot * 12, row);
        if (s.obs_in) {
            const int64_t M = s.agents;
            // obs[f] is also the state of transition f + M (f + M < n: in the window, one subtraction wraps there too)
            if (f + M < s.w.n) copy_row(a.ring.states + window_slot(s.w, f + M) * 12, state_after(f, row));
            if (f < M) copy_row(a.ring.states + slot * 12, s.obs_in + f * 12);
            else if (f - M < s.w.skip) copy_row(a.ring.states + slot * 12, state_after(f - M, s.next + (f - M) * 12));
        } else {
            copy_row(a.ring.states + slot * 12, s.states + f * 12);
        }
        a.ring.actions[slot] = s.actions[f];
        a.ring.rewards[slot] = s.rewards[f];
        if (a.ring.priorities) a.ring.priorities[slot] = top;
    }
}

// ---- the n-step add (uavtrack_replay_add_rollout_nstep; include/uavtrack.h has the definitions)

struct NstepArgs {
    AddArgs a;                                 // next: obs [steps][agents][12], rewards: reward [steps][agents]
    float *discounts;                          // [capacity]
    int n_step;
    float g;
};

// One thread per transition f = t * agents + b * n_uav + i, lanes consecutive in (b, i): for a fixed k the wavefront's
// reads of reward[t + k] are one line, and done[t + k][b] is shared by an environment's lanes.  A thread reads at most
// n_step - 1 done bytes and n_step rewards, its state row and the one obs row at the end of its window, and writes one
// transition.
__global__ void __launch_bounds__(kSW) replay_write_nstep_kernel(NstepArgs q)
{
#pragma clang fp contract(off)
    const ReplayRingView &ring = q.a.ring;
    const AddSource &a = q.a.s;
    const int64_t M = a.agents;
    const float top = ring.priorities ? *a.top : 0.0f;
    for (int64_t f = a.w.skip + (int64_t)blockIdx.x * kSW + threadIdx.x; f < a.w.n; f += (int64_t)gridDim.x * kSW) {
        const int64_t slot = window_slot(a.w, f);
        const int64_t t = f / M, r = f - t * M, b = r / a.n_uav;
        // the horizon: the smallest m >= 1 with m == n_step, t + m == steps or done[t + m - 1][b]
        const int64_t left = a.steps - t;
        const int lim = left < (int64_t)q.n_step ? (int)left : q.n_step;
        int m = 1;
        if (a.done) {
            const uint8_t *dn = a.done + t * a.envs + b;               // dn[k * envs] = done[t + k][b]
            while (m < lim && !dn[(int64_t)(m - 1) * a.envs]) ++m;
        } else {
            m = lim;
        }
        // the return, Horner from the far end, and the discount, m - 1 products
        const float *rw = a.rewards + f;                                // rw[k * M] = reward[t + k][b][i]
        float R = rw[(int64_t)(m - 1) * M], d = q.g;
        for (int k = m - 2; k >= 0; --k) {
            R = rw[(int64_t)k * M] + q.g * R;
            d = d * q.g;
        }
        const float *srow = a.obs_in + r * 12;
        if (t > 0) {
            const int64_t p = f - M;                                   // (t - 1, b, i)
            srow = (a.done && a.done[(t - 1) * a.envs + b]) ? a.start_obs + p * 12 : a.next + p * 12;
        }
        copy_row(ring.states + slot * 12, srow);
        copy_row(ring.next_states + slot * 12, a.next + (f + (int64_t)(m - 1) * M) * 12);
        ring.actions[slot] = a.actions[f];
        ring.rewards[slot] = R;
        q.discounts[slot] = d;
        if (ring.priorities) ring.priorities[slot] = top;
    }
}

// ---- the lambda add's scan (uavtrack_replay_add_rollout_lambda; include/uavtrack.h has the definitions)

struct LambdaArgs {
    AddSource s;                               // the write's own: the scan goes by the same window
    float *rewards, *discounts;                // the ring's [capacity] stores
    const float *values;                       // [steps][agents]
    float g, gl, c;                            // (float)gamma, g * l, g * (1 - l)
};

constexpr int kLambdaAhead = 8;                // steps per group: its loads are in flight while the group before it folds
constexpr int kLambdaW = 64;                   // threads per workgroup: a rollout has few chains (envs * n_uav), each a long
                                               // walk, so single-wavefront workgroups spread them over the most CUs

// One thread per agent chain r = b * n_uav + i, lanes consecutive in r: for a fixed t the wavefront's reads of reward[t]
// and values[t] are whole lines and its two stores are contiguous slots.  The loads do not depend on the carried G, so the
// walk is cut into groups of kLambdaAhead steps whose loads are unconditional and issued together, one group ahead of
// the fold (the steps beyond a multiple of kLambdaAhead, the rollout's last ones, go first, one at a time): a chain
// waits for memory once per group, not once per step.  The horizon is the whole rollout and nothing is kept per thread
// beyond two groups of kLambdaAhead steps.  WINDOW (the rollout exceeds the ring): rows before `skip` are walked (the
// walk has no other order) and not written; without it the fold is straight-line code.
template <bool DONE, bool WINDOW>
__global__ void __launch_bounds__(kLambdaW) replay_lambda_scan_kernel(LambdaArgs q)
{
#pragma clang fp contract(off)
    const AddSource &a = q.s;
    const int64_t M = a.agents, last = a.steps - 1;
    const float g = q.g, gl = q.gl, c = q.c;                           // (values: a select between two struct members
    const bool all_cut = gl == 0.0f;                                   //  would be a select of addresses and a load)
    for (int64_t r = (int64_t)blockIdx.x * kLambdaW + threadIdx.x; r < M; r += (int64_t)gridDim.x * kLambdaW) {
        const float *rw = a.rewards + r, *vv = q.values + r;            // rw[u * M] = reward[u][b][i]
        const uint8_t *dn = DONE ? a.done + r / a.n_uav : nullptr;      // dn[u * envs] = done[u][b]
        float G = 0.0f;
        auto fold = [&](int64_t u, float rew, float v, unsigned fired) {
            const bool cut = (u == last) | all_cut | (fired != 0);
            const float R = cut ? rew : rew + gl * G;
            const float d = cut ? g : c;
            G = R + d * v;
            const int64_t f = u * M + r;
            if (WINDOW && f < a.w.skip) return;
            const int64_t slot = window_slot(a.w, f);
            q.rewards[slot] = R;
            q.discounts[slot] = d;
        };
        // the three loads of step u, none of them conditional and nothing computed from them here
        auto load = [&](int64_t u, float &rew, float &v, unsigned &fired) {
            rew = rw[u * M];
            v = vv[u * M];
            fired = 0;
            if constexpr (DONE) fired = dn[u * a.envs];
        };
        int64_t t = a.steps;                                           // steps [0, t) are still to fold, t - 1 next
        for (int k = (int)(a.steps % kLambdaAhead); k > 0; --k) {
            --t;
            float rew, v;
            unsigned fired;
            load(t, rew, v, fired);
            fold(t, rew, v, fired);
        }
        if (t == 0) continue;
        // two groups in registers, A and B: while one folds, the loads of the group before it are in flight into the other
        // (at the front of the chain: the same group again, unused).  No group is ever copied: a copy would wait for it.
        struct Group { float rew[kLambdaAhead], v[kLambdaAhead]; unsigned fired[kLambdaAhead]; } A, B;
        auto load_group = [&](int64_t end, Group &grp) {               // steps [end - kLambdaAhead, end), last step first
#pragma unroll
            for (int q = 0; q < kLambdaAhead; ++q) load(end - 1 - q, grp.rew[q], grp.v[q], grp.fired[q]);
            __builtin_amdgcn_sched_barrier(0);                          // (the loads stay ahead of the fold behind them)
        };
        auto fold_group = [&](int64_t end, const Group &grp) {
#pragma unroll
            for (int q = 0; q < kLambdaAhead; ++q) fold(end - 1 - q, grp.rew[q], grp.v[q], grp.fired[q]);
            __builtin_amdgcn_sched_barrier(0);
        };
        load_group(t, A);
        while (true) {
            load_group(t > kLambdaAhead ? t - kLambdaAhead : t, B);
            fold_group(t, A);
            t -= kLambdaAhead;
            if (t == 0) break;
            load_group(t > kLambdaAhead ? t - kLambdaAhead : t, A);
            fold_group(t, B);
            t -= kLambdaAhead;
            if (t == 0) break;
        }
    }
}

// ---- the GAE add's scan (uavtrack_replay_add_rollout_gae; include/uavtrack.h has the definitions)

struct GaeArgs {
    LambdaArgs l;                              // the lambda scan's own: the same fold over the same window
    float *advantages;                         // [capacity], beside the ring
    const float *values_in;                    // [agents] V(obs_in)
    const float *values_start;                 // nullable with done: [steps][agents] V(start_obs), read where done fired
};

// The lambda scan's walk with one more load per step and three stores in place of two: the slot receives G_t itself
// (reward), +0.0f (discount) and G_t - V(s_t) (advantage).  V(s_t) is the value of the state step t began in: values_in at
// t == 0, else values[t - 1], a load that depends on nothing the fold carries and so travels in the step's group; where
// done[t - 1] fired it is values_start[t - 1] instead, one dependent load on the rare path.  Grouping, window and order
// of the fold are replay_lambda_scan_kernel's.
template <bool DONE, bool WINDOW>
__global__ void __launch_bounds__(kLambdaW) replay_gae_scan_kernel(GaeArgs p)
{
#pragma clang fp contract(off)
    const LambdaArgs &q = p.l;
    const AddSource &a = q.s;
    const int64_t M = a.agents, last = a.steps - 1;
    const float g = q.g, gl = q.gl, c = q.c;
    const bool all_cut = gl == 0.0f;
    for (int64_t r = (int64_t)blockIdx.x * kLambdaW + threadIdx.x; r < M; r += (int64_t)gridDim.x * kLambdaW) {
        const float *rw = a.rewards + r, *vv = q.values + r, *vin = p.values_in + r;
        const uint8_t *dn = DONE ? a.done + r / a.n_uav : nullptr;      // dn[u * envs] = done[u][b]
        float G = 0.0f;
        auto fold = [&](int64_t u, float rew, float v, unsigned fired, float vs, unsigned began) {
            const bool cut = (u == last) | all_cut | (fired != 0);
            const float R = cut ? rew : rew + gl * G;
            const float d = cut ? g : c;
            G = R + d * v;
            const int64_t f = u * M + r;
            if (WINDOW && f < a.w.skip) return;
            if (DONE && began) vs = p.values_start[f - M];              // (began != 0 only for u >= 1)
            const int64_t slot = window_slot(a.w, f);
            q.rewards[slot] = G;
            q.discounts[slot] = 0.0f;
            p.advantages[slot] = G - vs;
        };
        // the loads of step u, none of them conditional: the lambda scan's three, the value of the state before the step
        // and whether an episode ended there
        auto load = [&](int64_t u, float &rew, float &v, unsigned &fired, float &vs, unsigned &began) {
            rew = rw[u * M];
            v = vv[u * M];
            vs = *(u > 0 ? vv + (u - 1) * M : vin);
            fired = 0;
            began = 0;
            if constexpr (DONE) {
                fired = dn[u * a.envs];
                began = dn[(u > 0 ? u - 1 : 0) * a.envs];
                if (u == 0) began = 0;
            }
        };
        int64_t t = a.steps;                                           // steps [0, t) are still to fold, t - 1 next
        for (int k = (int)(a.steps % kLambdaAhead); k > 0; --k) {
            --t;
            float rew, v, vs;
            unsigned fired, began;
            load(t, rew, v, fired, vs, began);
            fold(t, rew, v, fired, vs, began);
        }
        if (t == 0) continue;
        struct Group {
            float rew[kLambdaAhead], v[kLambdaAhead], vs[kLambdaAhead];
            unsigned fired[kLambdaAhead], began[kLambdaAhead];
        } A, B;
        auto load_group = [&](int64_t end, Group &grp) {               // steps [end - kLambdaAhead, end), last step first
#pragma unroll
            for (int k = 0; k < kLambdaAhead; ++k)
                load(end - 1 - k, grp.rew[k], grp.v[k], grp.fired[k], grp.vs[k], grp.began[k]);
            __builtin_amdgcn_sched_barrier(0);                          // (the loads stay ahead of the fold behind them)
        };
        auto fold_group = [&](int64_t end, const Group &grp) {
#pragma unroll
            for (int k = 0; k < kLambdaAhead; ++k)
                fold(end - 1 - k, grp.rew[k], grp.v[k], grp.fired[k], grp.vs[k], grp.began[k]);
            __builtin_amdgcn_sched_barrier(0);
        };
        load_group(t, A);
        while (true) {
            load_group(t > kLambdaAhead ? t - kLambdaAhead : t, B);
            fold_group(t, A);
            t -= kLambdaAhead;
            if (t == 0) break;
            load_group(t > kLambdaAhead ? t - kLambdaAhead : t, A);
            fold_group(t, B);
            t -= kLambdaAhead;
            if (t == 0) break;
        }
    }
}

}  // namespace

// the maximum of the ring's priorities as they stand (1.0 for an empty ring) into d.parts[kReplayMaxParts]
static hipError_t launch_priority_top(const ReplayDevice &d, const ReplayRingView &ring, hipStream_t st)
{
    const int64_t cap = ring.capacity;
    int64_t groups = (cap + (int64_t)kSW * 16 - 1) / ((int64_t)kSW * 16);
    if (groups > kReplayMaxParts) groups = kReplayMaxParts;
    hipLaunchKernelGGL(replay_max_kernel, dim3((unsigned)groups), dim3(kSW), 0, st, ring.priorities, cap, d.parts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(replay_top_kernel, dim3(1), dim3(64), 0, st, d.parts, (int)groups, ring.count == 0 ? 1 : 0);
    return hipGetLastError();
}

hipError_t launch_replay_sample(const ReplayDevice &d, const float *priorities, int64_t count, int64_t k, float alpha,
                                double beta0, double beta1, int64_t anneal_calls, int64_t *indices, float *weights,
                                hipStream_t st)
{
    const int ntiles = (int)((count + kReplayTile - 1) / kReplayTile);
    hipLaunchKernelGGL(replay_begin_kernel, dim3(1), dim3(64), 0, st, d.counter, d.status, d.pmin);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(replay_tile_kernel, dim3(ntiles), dim3(kSW), 0, st, priorities, count, alpha, d.prefix,
                       d.tile_last, d.status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(replay_scan_kernel, dim3(1), dim3(kScanW), 0, st, d.prefix, ntiles, d.status, d.errors);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    DrawArgs a;
    a.prio = priorities; a.prefix = d.prefix; a.tile_last = d.tile_last; a.counter = d.counter; a.status = d.status;
    a.pdraw = d.pdraw; a.indices = indices; a.count = count; a.k = k; a.ntiles = ntiles;
    a.alpha = alpha; a.k0 = d.k0; a.k1 = d.k1;
    const int64_t per = kSW / 64;
    hipLaunchKernelGGL(replay_draw_kernel, dim3((unsigned)((k + per - 1) / per)), dim3(kSW), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (weights) {
        int64_t mg = (k + (int64_t)kSW * 16 - 1) / ((int64_t)kSW * 16);
        if (mg > 1024) mg = 1024;
        hipLaunchKernelGGL(replay_min_kernel, dim3((unsigned)mg), dim3(kSW), 0, st, d.pdraw, k, d.pmin);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(replay_weight_kernel, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, st, d.pdraw, k, count,
                           beta0, beta1, anneal_calls, d.counter, d.pmin, d.status, weights);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

// half the width of the walk's domain: the width even, >= 2, count <= 2^width (< 4 * count from count 2 on)
static int walk_half_bits(int64_t count)
{
    static_assert(kUniformRounds % 4 == 0, "round keys come in Philox blocks of four");
    int bits = 2;
    while (((int64_t)1 << bits) < count) bits += 2;
    return bits / 2;
}

hipError_t launch_replay_sample_uniform(const ReplayDevice &d, int64_t count, int64_t k, int64_t *indices, hipStream_t st)
{
    hipLaunchKernelGGL(replay_begin_kernel, dim3(1), dim3(64), 0, st, d.counter, d.status, d.pmin);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(replay_uniform_kernel, dim3((unsigned)((k + kSW - 1) / kSW)), dim3(kSW), 0, st, d.counter, count,
                       k, walk_half_bits(count), d.k0, d.k1, indices);
    return hipGetLastError();
}

hipError_t launch_replay_sample_sweep(const ReplayDevice &d, int64_t capacity, int64_t first, int64_t length, int64_t n,
                                      uint64_t *cursor, int64_t *indices, hipStream_t st)
{
    hipLaunchKernelGGL(replay_cursor_kernel, dim3(1), dim3(64), 0, st, cursor);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    SweepArgs a;
    a.cursor = cursor; a.indices = indices; a.first = first; a.length = length; a.n = n; a.cap = capacity;
    a.half = walk_half_bits(length); a.k0 = d.k0; a.k1 = d.k1;
    hipLaunchKernelGGL(replay_sweep_kernel, dim3((unsigned)((n + kSW - 1) / kSW)), dim3(kSW), 0, st, a);
    return hipGetLastError();
}

// `kernel` over `items` threads' worth of work in workgroups of `threads` (the kernels stride beyond 65536 workgroups)
template <class Kernel, class Args>
static hipError_t launch_over(Kernel kernel, int64_t items, int threads, hipStream_t st, const Args &a)
{
    int64_t blocks = (items + threads - 1) / threads;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(threads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_replay_add(const ReplayDevice &d, const ReplayAdd &q, hipStream_t st)
{
    hipError_t e;
    if (q.ring.priorities && (e = launch_priority_top(d, q.ring, st)) != hipSuccess) return e;
    AddArgs a;
    AddSource &s = a.s;
    a.ring = q.ring; s.obs_in = q.obs_in; s.states = q.states; s.next = q.next; s.actions = q.actions;
    s.rewards = q.rewards; s.done = q.done; s.start_obs = q.start_obs; s.top = d.parts + kReplayMaxParts;
    s.envs = q.envs; s.n_uav = q.n_uav; s.steps = q.steps; s.agents = q.envs * q.n_uav;
    s.w = ring_window(q.ring, q.steps * s.agents);             // what the write and the lambda scan both go by
    const int64_t written = s.w.n - s.w.skip;
    if (q.form == ReplayForm::Nstep) {
        NstepArgs n;
        n.a = a; n.discounts = q.discounts; n.n_step = q.n_step; n.g = q.gamma;
        return launch_over(replay_write_nstep_kernel, written, kSW, st, n);
    }
    // lambda: states, actions, next states and priorities (and the raw rewards, which the scan overwrites) as the one-step add
    e = q.done ? launch_over(replay_write_kernel<true>, written, kSW, st, a)
               : launch_over(replay_write_kernel<false>, written, kSW, st, a);
    if ((q.form != ReplayForm::Lambda && q.form != ReplayForm::Gae) || e != hipSuccess) return e;
    LambdaArgs l;
    l.s = s; l.rewards = q.ring.rewards; l.discounts = q.discounts; l.values = q.values;
    l.g = q.gamma;
    l.gl = q.gamma * q.lambda;
    l.c = q.gamma * (1.0f - q.lambda);
    const bool window = s.w.skip != 0;
    if (q.form == ReplayForm::Gae) {
        GaeArgs p;
        p.l = l; p.advantages = q.advantages; p.values_in = q.values_in; p.values_start = q.values_start;
        auto gae = q.done ? (window ? replay_gae_scan_kernel<true, true> : replay_gae_scan_kernel<true, false>)
                          : (window ? replay_gae_scan_kernel<false, true> : replay_gae_scan_kernel<false, false>);
        return launch_over(gae, s.agents, kLambdaW, st, p);
    }
    auto scan = q.done ? (window ? replay_lambda_scan_kernel<true, true> : replay_lambda_scan_kernel<true, false>)
                       : (window ? replay_lambda_scan_kernel<false, true> : replay_lambda_scan_kernel<false, false>);
    return launch_over(scan, s.agents, kLambdaW, st, l);
}

}  // namespace uavtrack

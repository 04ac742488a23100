// learner_kernel.hip -- ActorCritic.update (actor_critic.py:150-179) and both torch.optim.Adam steps on the device,
// plus the PrioritizedReplayBuffer.update_priorities write of train.py:262 (train.py:136-138).
//
// One update is a chain of stream-ordered launches (a one-thread kernel clears the status word first), none of which synchronises or allocates:
//   learner_grad_kernel      rows gathered through the index vector, tiled R rows at a time per workgroup: both
//                            forwards (critic on s and s', actor on s), softmax, TD error, both backwards; every
//                            gradient sum of the tile is added into the workgroup's LDS accumulators (each
//                            parameter owned by one thread, so the order of the adds is fixed), and the workgroup
//                            writes one partial row [P + 4] (gradients, then the four loss sums) at the end;
//   learner_finalize_kernel  the loss partials summed in workgroup order -> losses, gradient scales, step counters;
//   learner_adam_kernel      per parameter: the gradient partials summed in workgroup order, scaled, Adam;
//   learner_prio_*           |delta| into the priorities at the sampled slots, the last occurrence of a slot in the
//                            batch winning (a claim / max-row / mark / write chain: no float atomics anywhere).
// Nothing depends on timing, so two identical calls give bitwise identical results.
// The split form cuts the same chain after the sums: learner_reduce_kernel leaves them in a gradient row, and the apply
// runs the same finalize and Adam kernels over rows instead of workgroup partials (see below).
//
// The sums are arranged so the reference's broadcast actor loss costs nothing extra: with
// actor_loss = mean_i(-log p_i) * mean_j(delta_j), dL/dz_i = -mean(delta) (onehot(a_i) - p_i) / n, so the grad kernel
// accumulates (onehot - p) and the Adam kernel multiplies by -mean(delta) / n once.  Per-sample: delta_i (onehot - p)
// is accumulated and scaled by -1 / n.  The critic accumulates (V - target) and is scaled by 2 / n.
//
// Importance weights (uavtrack_learner_update_weighted / _grad_weighted): row i carries w_i >= 0 and the losses become
// critic mean_i(w_i (V - y)^2), per-sample actor mean_i(-w_i log p_i delta_i), reference actor
// mean_i(-w_i log p_i) * mean_j(w_j delta_j) -- the pair (i, j) of the broadcast loss weighted by w_i w_j.  Every sum
// above takes its row's w_i as one more factor (the logit weight, the value weight, the four loss terms) and nothing
// after the sums changes: the means still divide by n, and -(sum w delta / N) / N falls out of the same words.  No
// weights is the factor 1.0f, an exact multiply, so the unweighted update keeps its bits.
//
// Per-row discounts (uavtrack_learner_update_discounted / _grad_discounted): the target of row i is y_i = r_i + d_i V(s'_i)
// with d_i read from a per-slot store through the row's index, beside the reward (an n-step ring keeps gamma^m there).
// The tile gather leaves d_i in LDS; no store is d_i = gamma for every row, the same multiply as before.
//
// Regularisation (uavtrack_learner_set_regularisation, off by default).  An entropy bonus c > 0 (per-sample form only)
// makes the actor loss mean_i(w_i (-log p_i delta_i - c H_i)), H_i = -sum_o p_io log p_io: the accumulated logit weight
// of a row becomes w_i (delta_i (onehot - p_i)_o - c p_io (log p_io + H_i)), still scaled by -1 / N afterwards, and loss
// word 2 carries the whole term, so rows keep their layout and still add.  Every log p then comes from the logits,
// (z_o - max) - log sum exp, never from logf(p): finite for every finite logit vector.  learner_grad_reg_kernel is the
// same body compiled with that block; learner_grad_kernel stays what it was.  Gradient-norm clipping (one max_norm per
// network) runs between "scale" and "Adam": learner_gradsum_kernel forms the scaled gradient once and leaves each
// workgroup's sums of squares in fp64, learner_clip_kernel adds them in workgroup order and writes both coefficients,
// and the same Adam kernel then runs over (the scaled gradient, count 1, the coefficients as its scales).
//
// The target critic (uavtrack_learner_set_target, off by default): a second copy of the critic's 14 H + 1 words from which
// V(s') alone is formed, y_i = r_i + d_i V_target(s'_i); V(s_i), both backward passes and everything behind delta are
// unchanged.  learner_grad_target_kernel / learner_grad_reg_target_kernel are the same body with the layer-1 and layer-2
// chains of V(s') over the other block (read from global memory, as the online weights are: no more LDS);
// learner_target_kernel, behind the Adam kernel and gated on the same status word, moves the block towards the critic
// (Polyak) or copies it every `period` steps of the device step counter.  While off, the launches are the ones above.
//
// The clipped surrogate (uavtrack_learner_update_clipped / _grad_clipped, per-sample form only): the ratio
// r_i = expf(log p_i - log_mu[src_i]) against a per-slot store of behaviour log-probabilities is differentiated through,
// and a row's policy gradient stops once r_i has left [lo, hi] in the direction its advantage delta_i pushes:
// pass_i = delta_i >= 0 ? r_i <= hi : r_i >= lo, surr_i = min(r delta, clip(r, lo, hi) delta), logit weight
// w_i ((pass_i ? delta_i r_i : 0) (onehot - p_i)_o - c p_io (log p_io + H_i)), loss word 2 sum w_i (-surr_i - c H_i).
// learner_grad_clip_kernel / _clip_target_kernel are the same body with that block (kClip), always on the logits path;
// the tile gather leaves log_mu[src] in R more floats of LDS behind dc, so only these two ask for the larger allocation.
// log p_i is (z_a - max) - logf(sum expf(z - max)), the bits of learner_policy_kernel, and expf(0.0f) == 1.0f, so a row
// whose log_mu holds those bits trains with the bits of the per-sample row.  A drawn slot whose log_mu is NaN or > 0, or
// whose r_i is not finite, sets status bit 4 (value 16) and is not used.
//
// Batch-normalised advantages (uavtrack_learner_set_advantage, per-sample form only, off by default): the advantage that
// multiplies grad log p, gates the clip and enters the actor loss becomes A_i = fl(fl(delta_i - mean) * inv_std), mean and
// inv_std read from three floats of device memory; the critic, td_delta, loss word 1 and the priorities keep delta_i.
// learner_grad_adv_kernel and its three siblings are the same body with that line (kAdv), reading the pair through
// GradArgs::stats; the other six never read that field.  In batch mode three small kernels run in front:
// learner_td_kernel forms delta_i of every row by the gradient kernel's own chains (the bits it will form) and each
// 256-row chunk's fp64 sum, learner_adv_sq_kernel each chunk's sum of squared deviations, learner_adv_stats_kernel the
// three floats; learner_adv_seal_kernel, behind the gradient kernel, turns them into NaN where the update was refused.
//
// Which of the fourteen instantiations of the gradient body a launch takes is learner_variants.h's table and its
// learner_grad_variant; the host code below expands the same table over the kernels (kGradKernels), prepares every row's
// LDS attribute from it and launches through it.  Every kernel takes the one GradArgs, filled whole by launch_grad, and
// reads of it what its flags compile in.
//
// Stored advantages (uavtrack_learner_update_stored / _grad_stored, per-sample form only): the advantage the actor starts
// from is x_i = advantages[src_i], a per-slot store gathered beside the reward (a GAE ring's seventh store), in delta_i's
// place wherever the actor uses an advantage; the advantage mode applies on top, A_i = fl(fl(x_i - mean) * inv_std), raw
// being the handle's constant pair {0, 1}.  The critic, td_delta, loss word 1 and the priorities keep delta_i.  Four more
// instantiations of the body (kStored; always kReg and kAdv, by kTgt and kClip), the last four rows of the table in
// learner_variants.h; the ten above never read GradArgs::advantages.  In batch mode learner_adv_gather_kernel writes
// x_i into the TD scratch in learner_td_kernel's place and the statistics kernels run over it unchanged.  A drawn
// advantage that is NaN or infinite sets status bit 7 (value 128) and the row is not used.
//
// KL early stopping (uavtrack_learner_set_kl_stop, closed clipped updates only, off by default): behind the gradient kernel
// learner_kl_chunk_kernel sums k_i = (r_i - 1) - log r_i of the ratios in fp64 per 256-row chunk and learner_kl_kernel forms
// kl = (float)(sum / n), and where kl > limit sets a latch in the caller's device memory and status bit 8 (value 256): the
// update is stopped -- everything gated on the status word skips it, the finalize kernel counts no error -- and so is
// every update behind it until the latch is reset: learner_begin_kl_kernel starts such an update's status word at 256, and
// the kClip instantiations read the latch through GradArgs::latch and return before the first tile.  While off, the
// launches and their arguments are the ones above (GradArgs::latch null).
//
// The critic alone (uavtrack_learner_values): learner_values_kernel, at the end of the kernels below, evaluates V(x) of
// any number of rows by the chain of the layer-1 and layer-2 loops above, to the bit, and touches no learner state.

#include "learner.h"
#include "learner_variants.h"

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

namespace uavtrack {

namespace {

constexpr int kLW = 256;   // threads per workgroup of the grad kernel

// The launch's shape, folded on the host: one struct for all fourteen kernels.  Every kernel reads the fields down to
// `target`; behind them a field is read only under the flag its comment names, and a kernel compiled without that flag
// holds no load of it.
struct GradArgs {
    const float *params;            // [P] both networks, LearnerLayout order
    const float *states, *rewards, *next_states;
    const int32_t *actions;
    const int64_t *idx;             // nullable: rows 0..n-1
    const float *weights;           // nullable [n], batch order: importance weights (null: every row 1.0f)
    int64_t n, capacity;
    float *partials;                // [groups][P + 4]
    float *td_delta;                // nullable [n]
    int *status;                    // bit 0: action out of range, bit 1: index out of range, bit 2: weight NaN, inf or < 0
                                    // (bit 3: a bad discount, below; bit 4: a bad log_mu or ratio, further below)
    LearnerLayout L;
    int rows;                       // R rows per tile
    float gamma;
    int per_sample;
    float entropy_coef;             // c >= 0 (learner_grad_reg_kernel only; c != 0 only with per_sample)
    float *entropy;                 // nullable [n]: H_i of batch row i, 0 for a row that was not used
    const float *discounts;         // nullable [capacity], slot order: the row's discount d in y = r + d V(s') (null: gamma);
                                    // status bit 3: a discount that is NaN, negative or above 1
    const float *target;            // the target critic's block [14 H + 1] at its own offsets 0, 12 H, 13 H, 14 H
                                    // (read under kTgt; null otherwise)
    // read under kClip (the clipped surrogate):
    const float *log_mu;            // [capacity], slot order: behaviour log-probabilities; status bit 4: a drawn slot whose
                                    // log_mu is NaN or > 0, or whose ratio is not finite
    float clip_lo, clip_hi;         // 1 - eps, 1 + eps in fp32, folded on the host
    float *ratio;                   // nullable [n]: r_i of batch row i, NaN for a row that set a status bit
    // read under kAdv (a normalised advantage, and every stored one):
    const float *stats;             // [2] {mean, inv_std}, read when the launch executes; status bit 6 (value 64): a mean
                                    // that is not finite, or an inv_std that is NaN, infinite or negative
    // read under kStored:
    const float *advantages;        // [capacity], slot order: the actor's advantage x_i of a row, in delta_i's place; status
                                    // bit 7 (value 128): a drawn slot whose advantage is NaN or infinite
    // read under kClip, at the top of the body (KL early stopping):
    const int32_t *latch;           // nullable [1]: the KL latch; non-zero when the launch executes: the launch does nothing
};

// kReg: the entropy term and the entropy[] store in the per-row block; everything else is one text.
// kTgt: V(s') from the separate critic block a.target (the target critic) instead of the online critic; without it
// W1t / b1t / W2t / b2t are the online critic's pointers at compile time.
// kClip (with kReg): the clipped surrogate's gate on the row's policy gradient, log_mu gathered into lm, the ratio[] store.
// kAdv (with kReg): the row's advantage is fl(fl(delta - mean) * inv_std) wherever the actor uses one.
// kStored (with kAdv): the advantage the line above starts from is advantages[src], gathered into xa, not delta.
template <bool kReg, bool kTgt = false, bool kClip = false, bool kAdv = false, bool kStored = false>
__device__ __forceinline__ void learner_grad_body(const GradArgs &a)
{
    static_assert(kReg || !kAdv, "the normalised advantage lives in the kReg block");
    static_assert(kAdv || !kStored, "a stored advantage passes through the normalised advantage's line");
    // KL early stopping: a latched learner's update is thrown away, so it is not formed.  One word through a kernel
    // argument: the same for every lane of every workgroup, ahead of the first barrier.
    if constexpr (kClip)
        if (a.latch && *a.latch) return;
    extern __shared__ float lds[];
    const LearnerLayout &L = a.L;
    const int H = L.H, A = L.A, R = a.rows, P = L.P;
    float *acc = lds;                       // [P]
    float *s   = acc + P;                   // [R][12]
    float *s2  = s + R * 12;                // [R][12]
    float *ha  = s2 + R * 12;               // [R][H]  actor hidden (post-ReLU)
    float *hc  = ha + R * H;                // [R][H]  critic hidden on s
    float *hx  = hc + R * H;                // [R][H]  critic hidden on s', then the actor's dL/dh
    float *gz  = hx + R * H;                // [R][A]  logits, then the accumulated logit weights
    float *gv  = gz + R * A;                // [R]     V, then (V - target)
    float *vn  = gv + R;                    // [R]     V'
    float *lt  = vn + R;                    // [R][4]  per-row loss terms
    int *act   = reinterpret_cast<int *>(lt + R * 4);   // [R] action, -1 = row not used
    float *wt  = reinterpret_cast<float *>(act + R);    // [R] importance weight of the row
    float *dc  = wt + R;                                // [R] discount of the row
    float *lm  = dc + R;                                // [R] behaviour log-probability of the row (kClip only)
    float *xa  = lm + R;                                // [R] stored advantage of the row (kStored only)

    const int tid = threadIdx.x;
    const float *W1a = a.params + L.a_w1, *b1a = a.params + L.a_b1, *W2a = a.params + L.a_w2, *b2a = a.params + L.a_b2;
    const float *W1c = a.params + L.c_w1, *b1c = a.params + L.c_b1, *W2c = a.params + L.c_w2, *b2c = a.params + L.c_b2;
    const float *W1t = kTgt ? a.target : W1c, *b1t = kTgt ? a.target + 12 * H : b1c;
    const float *W2t = kTgt ? a.target + 13 * H : W2c, *b2t = kTgt ? a.target + 14 * H : b2c;

    float adv_mean = 0.0f, adv_inv = 1.0f;
    bool adv_bad = false;
    if constexpr (kAdv) {
        adv_mean = a.stats[0]; adv_inv = a.stats[1];
        adv_bad = !(fabsf(adv_mean) <= 3.402823466e+38f) || !(adv_inv >= 0.0f && adv_inv <= 3.402823466e+38f);
    }

    for (int p = tid; p < P; p += kLW) acc[p] = 0.0f;
    float loss_run[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // thread 0's running sums, tile after tile

    const int64_t tiles = (a.n + R - 1) / R;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        // ---- gather the tile: states, next states, action, reward, discount, importance weight
        for (int r = tid; r < R; r += kLW) {
            const int64_t i = row0 + r;
            int av = -1;
            float wi = 1.0f, di = a.gamma;
            if (i < a.n) {
                const int64_t src = a.idx ? a.idx[i] : i;
                if (src < 0 || src >= a.capacity) {
                    atomicOr(a.status, 2);
                } else {
                    av = a.actions[src];
                    if (av < 0 || av >= A) { atomicOr(a.status, 1); av = -1; }
                    vn[r] = a.rewards[src];               // the reward waits in vn until V' overwrites it
                    if (a.discounts) {
                        di = a.discounts[src];
                        if (!(di >= 0.0f && di <= 1.0f)) { atomicOr(a.status, 8); av = -1; }
                    }
                    if constexpr (kClip) {
                        const float mu = a.log_mu[src];
                        if (!(mu <= 0.0f)) { atomicOr(a.status, 16); av = -1; }
                        lm[r] = mu;
                    }
                    if constexpr (kStored) {
                        const float x = a.advantages[src];
                        if (!(fabsf(x) <= 3.402823466e+38f)) { atomicOr(a.status, 128); av = -1; }
                        xa[r] = x;
                    }
                }
                if (a.weights) {
                    wi = a.weights[i];
                    if (!(wi >= 0.0f) || isinf(wi)) { atomicOr(a.status, 4); av = -1; }
                }
                if constexpr (kAdv)
                    if (adv_bad) { atomicOr(a.status, 64); av = -1; }
                for (int k = 0; k < 12; ++k) {
                    s[r * 12 + k]  = av >= 0 ? a.states[src * 12 + k] : 0.0f;
                    s2[r * 12 + k] = av >= 0 ? a.next_states[src * 12 + k] : 0.0f;
                }
            } else {
                for (int k = 0; k < 12; ++k) { s[r * 12 + k] = 0.0f; s2[r * 12 + k] = 0.0f; }
            }
            if (av < 0) vn[r] = 0.0f;
            act[r] = av;
            wt[r] = wi;
            dc[r] = di;
        }
        __syncthreads();
        // ---- layer 1 of the three forwards
        for (int e = tid; e < R * H; e += kLW) {
            const int r = e / H, j = e - r * H;
            float pa = b1a[j], pc = b1c[j], pn = b1t[j];
            for (int k = 0; k < 12; ++k) {
                pa = fmaf(W1a[j * 12 + k], s[r * 12 + k], pa);
                pc = fmaf(W1c[j * 12 + k], s[r * 12 + k], pc);
                pn = fmaf(W1t[j * 12 + k], s2[r * 12 + k], pn);
            }
            ha[e] = fmaxf(pa, 0.0f);
            hc[e] = fmaxf(pc, 0.0f);
            hx[e] = fmaxf(pn, 0.0f);
        }
        __syncthreads();
        // ---- layer 2: A logits, V, V' per row (the reward moves from vn to lt[.][0] first)
        for (int r = tid; r < R; r += kLW) lt[r * 4] = vn[r];
        __syncthreads();
        const int O = A + 2;
        for (int e = tid; e < R * O; e += kLW) {
            const int r = e / O, o = e - r * O;
            const float *h = o < A ? ha + r * H : (o == A ? hc + r * H : hx + r * H);
            const float *w = o < A ? W2a + o * H : (o == A ? W2c : W2t);
            float z = o < A ? b2a[o] : (o == A ? b2c[0] : b2t[0]);
            for (int j = 0; j < H; ++j) z = fmaf(w[j], h[j], z);
            if (o < A) gz[r * A + o] = z;
            else if (o == A) gv[r] = z;
            else vn[r] = z;
        }
        __syncthreads();
        // ---- per row: softmax, log p_a, TD error, the logit and value weights of the backward pass
        for (int r = tid; r < R; r += kLW) {
            const int av = act[r];
            const float rew = lt[r * 4];
            float *z = gz + r * A;
            if (av < 0) {
                for (int o = 0; o < A; ++o) z[o] = 0.0f;
                gv[r] = 0.0f;
                lt[r * 4 + 0] = lt[r * 4 + 1] = lt[r * 4 + 2] = lt[r * 4 + 3] = 0.0f;
                if (kReg && a.entropy && row0 + r < a.n) a.entropy[row0 + r] = 0.0f;
                if constexpr (kClip)
                    if (a.ratio && row0 + r < a.n) a.ratio[row0 + r] = NAN;
                continue;
            }
            float m = z[0];
            for (int o = 1; o < A; ++o) m = fmaxf(m, z[o]);
            if constexpr (kReg) {
                // d_o = z_o - max stays in z; e_o = expf(d_o) is formed again where it is needed (the same bits).
                // H = log sum e - (sum e_o d_o) / sum e: both terms >= 0, and e_o == 0 (an underflowed probability)
                // contributes 0, not 0 * d_o.
                float sum = 0.0f, sd = 0.0f;
                for (int o = 0; o < A; ++o) {
                    const float d = z[o] - m, e = expf(d);
                    z[o] = d;
                    sum += e;
                    sd += e > 0.0f ? e * d : 0.0f;
                }
                const float inv = 1.0f / sum;
                const float lse = logf(sum);
                const float ent = lse - sd * inv;
                const float target = rew + dc[r] * vn[r];
                const float v = gv[r];
                const float delta = target - v;
                float adv = delta;                                  // the actor's advantage; delta stays the critic's
                if constexpr (kStored) adv = xa[r];
                if constexpr (kAdv) adv = __fmul_rn(__fsub_rn(adv, adv_mean), adv_inv);
                const float wi = wt[r];
                const float c = a.entropy_coef;
                float nlp, al;
                if constexpr (kClip) {
                    nlp = lse - z[av];
                    const float ratio = expf((z[av] - lse) - lm[r]);
                    if (!(ratio <= 3.402823466e+38f)) {             // inf or NaN: the row is not used
                        atomicOr(a.status, 16);
                        for (int o = 0; o < A; ++o) z[o] = 0.0f;
                        gv[r] = 0.0f;
                        lt[r * 4 + 0] = lt[r * 4 + 1] = lt[r * 4 + 2] = lt[r * 4 + 3] = 0.0f;
                        if (a.entropy) a.entropy[row0 + r] = 0.0f;
                        if (a.ratio) a.ratio[row0 + r] = NAN;
                        continue;
                    }
                    const bool pass = adv >= 0.0f ? ratio <= a.clip_hi : ratio >= a.clip_lo;
                    const float dr = pass ? adv * ratio : 0.0f;     // ratio == 1: the advantage's bits
                    const float surr = pass ? dr : (adv >= 0.0f ? a.clip_hi : a.clip_lo) * adv;
                    if (c != 0.0f) {                                // launch-uniform
                        for (int o = 0; o < A; ++o) {
                            const float d = z[o], e = expf(d), p = e * inv;
                            const float ge = e > 0.0f ? p * ((d - lse) + ent) : 0.0f;
                            z[o] = wi * (dr * ((o == av ? 1.0f : 0.0f) - p) - c * ge);
                        }
                        al = wi * (-surr - c * ent);
                    } else {
                        const float w = dr * wi;
                        for (int o = 0; o < A; ++o) z[o] = w * ((o == av ? 1.0f : 0.0f) - expf(z[o]) * inv);
                        al = -surr * wi;
                    }
                    if (a.ratio) a.ratio[row0 + r] = ratio;
                } else if (c != 0.0f) {                             // launch-uniform
                    nlp = lse - z[av];
                    for (int o = 0; o < A; ++o) {
                        const float d = z[o], e = expf(d), p = e * inv;
                        const float ge = e > 0.0f ? p * ((d - lse) + ent) : 0.0f;
                        z[o] = wi * (adv * ((o == av ? 1.0f : 0.0f) - p) - c * ge);
                    }
                    al = wi * (nlp * adv - c * ent);
                } else {                                            // today's values, to the bit
                    nlp = -logf(expf(z[av]) * inv);
                    const float w = (a.per_sample ? adv : 1.0f) * wi;
                    for (int o = 0; o < A; ++o) z[o] = w * ((o == av ? 1.0f : 0.0f) - expf(z[o]) * inv);
                    al = (nlp * adv) * wi;
                }
                gv[r] = (v - target) * wi;
                lt[r * 4 + 0] = nlp * wi;
                lt[r * 4 + 1] = delta * wi;
                lt[r * 4 + 2] = al;
                lt[r * 4 + 3] = ((v - target) * (v - target)) * wi;
                if (a.td_delta) a.td_delta[row0 + r] = delta;
                if (a.entropy) a.entropy[row0 + r] = ent;
                continue;
            }
            float sum = 0.0f;
            for (int o = 0; o < A; ++o) { z[o] = expf(z[o] - m); sum += z[o]; }
            const float inv = 1.0f / sum;
            const float target = rew + dc[r] * vn[r];
            const float v = gv[r];
            const float delta = target - v;
            const float nlp = -logf(z[av] * inv);
            const float wi = wt[r];
            const float w = (a.per_sample ? delta : 1.0f) * wi;
            for (int o = 0; o < A; ++o) z[o] = w * ((o == av ? 1.0f : 0.0f) - z[o] * inv);
            gv[r] = (v - target) * wi;
            lt[r * 4 + 0] = nlp * wi;
            lt[r * 4 + 1] = delta * wi;
            lt[r * 4 + 2] = (nlp * delta) * wi;
            lt[r * 4 + 3] = ((v - target) * (v - target)) * wi;
            if (a.td_delta) a.td_delta[row0 + r] = delta;
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < R; ++r)
                for (int q = 0; q < 4; ++q) loss_run[q] += lt[r * 4 + q];
        // ---- the actor's dL/dh (up to the -scale / n of the Adam kernel), masked by its ReLU; over hx
        for (int e = tid; e < R * H; e += kLW) {
            const int r = e / H, j = e - r * H;
            float d = 0.0f;
            if (ha[e] > 0.0f)
                for (int o = 0; o < A; ++o) d = fmaf(W2a[o * H + j], gz[r * A + o], d);
            hx[e] = d;
        }
        __syncthreads();
        // ---- the tile's gradient sums into the accumulators, one owner thread per parameter, rows in order
        for (int p = tid; p < 12 * H; p += kLW) {           // actor fc1.weight [H][12]
            const int j = p / 12, k = p - j * 12;
            float g = acc[L.a_w1 + p];
            for (int r = 0; r < R; ++r) g = fmaf(hx[r * H + j], s[r * 12 + k], g);
            acc[L.a_w1 + p] = g;
        }
        for (int j = tid; j < H; j += kLW) {                // actor fc1.bias, critic fc1.bias, critic fc2.weight
            float ga = acc[L.a_b1 + j], gb = acc[L.c_b1 + j], gw = acc[L.c_w2 + j];
            const float w2 = W2c[j];
            for (int r = 0; r < R; ++r) {
                ga += hx[r * H + j];
                gb += hc[r * H + j] > 0.0f ? gv[r] * w2 : 0.0f;
                gw = fmaf(gv[r], hc[r * H + j], gw);
            }
            acc[L.a_b1 + j] = ga; acc[L.c_b1 + j] = gb; acc[L.c_w2 + j] = gw;
        }
        for (int p = tid; p < A * H; p += kLW) {            // actor fc2.weight [A][H]
            const int o = p / H, j = p - o * H;
            float g = acc[L.a_w2 + p];
            for (int r = 0; r < R; ++r) g = fmaf(gz[r * A + o], ha[r * H + j], g);
            acc[L.a_w2 + p] = g;
        }
        for (int o = tid; o < A; o += kLW) {                // actor fc2.bias
            float g = acc[L.a_b2 + o];
            for (int r = 0; r < R; ++r) g += gz[r * A + o];
            acc[L.a_b2 + o] = g;
        }
        for (int p = tid; p < 12 * H; p += kLW) {           // critic fc1.weight [H][12]
            const int j = p / 12, k = p - j * 12;
            float g = acc[L.c_w1 + p];
            const float w2 = W2c[j];
            for (int r = 0; r < R; ++r)
                if (hc[r * H + j] > 0.0f) g = fmaf(gv[r] * w2, s[r * 12 + k], g);
            acc[L.c_w1 + p] = g;
        }
        if (tid == 0) {                                     // critic fc2.bias
            float g = acc[L.c_b2];
            for (int r = 0; r < R; ++r) g += gv[r];
            acc[L.c_b2] = g;
        }
        __syncthreads();
    }
    float *out = a.partials + (size_t)blockIdx.x * (P + 4);
    for (int p = tid; p < P; p += kLW) out[p] = acc[p];
    if (tid == 0)
        for (int q = 0; q < 4; ++q) out[P + q] = loss_run[q];
}

__global__ void __launch_bounds__(kLW) learner_grad_kernel(GradArgs a) { learner_grad_body<false>(a); }

// launched instead of learner_grad_kernel while entropy_coef != 0 or an entropy[] buffer is installed
__global__ void __launch_bounds__(kLW) learner_grad_reg_kernel(GradArgs a) { learner_grad_body<true>(a); }

// the same two while a target critic is enabled (uavtrack_learner_set_target): V(s') over a.target
__global__ void __launch_bounds__(kLW) learner_grad_target_kernel(GradArgs a) { learner_grad_body<false, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_reg_target_kernel(GradArgs a) { learner_grad_body<true, true>(a); }

// the clipped surrogate (uavtrack_learner_update_clipped / _grad_clipped), without and with a target critic
__global__ void __launch_bounds__(kLW) learner_grad_clip_kernel(GradArgs a) { learner_grad_body<true, false, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_clip_target_kernel(GradArgs a) { learner_grad_body<true, true, true>(a); }

// the normalised advantage (uavtrack_learner_set_advantage), without and with the clipped surrogate and a target critic
__global__ void __launch_bounds__(kLW) learner_grad_adv_kernel(GradArgs a) { learner_grad_body<true, false, false, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_adv_target_kernel(GradArgs a) { learner_grad_body<true, true, false, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_adv_clip_kernel(GradArgs a) { learner_grad_body<true, false, true, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_adv_clip_target_kernel(GradArgs a) { learner_grad_body<true, true, true, true>(a); }

// a stored advantage (uavtrack_learner_update_stored / _grad_stored), without and with the clipped surrogate and a target critic
__global__ void __launch_bounds__(kLW) learner_grad_stored_kernel(GradArgs a) { learner_grad_body<true, false, false, true, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_stored_target_kernel(GradArgs a) { learner_grad_body<true, true, false, true, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_stored_clip_kernel(GradArgs a) { learner_grad_body<true, false, true, true, true>(a); }
__global__ void __launch_bounds__(kLW) learner_grad_stored_clip_target_kernel(GradArgs a) { learner_grad_body<true, true, true, true, true>(a); }

// Clears the update's status word (a kernel node rather than a memset node, so a captured update is a chain of kernels)
__global__ void learner_begin_kernel(int *status)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *status = 0;
}

// In learner_begin_kernel's place while KL early stopping is on: a latched learner's update starts stopped, so every
// kernel gated on the status word skips it.
__global__ void learner_begin_kl_kernel(int *status, const int32_t *kl_state)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) *status = kl_state[0] ? kLearnerStopped : 0;
}

// The ordered sum every reduction over partial rows or gradient rows uses: word p of `count` rows, rows ascending.
__device__ __forceinline__ float ordered_sum(const float *src, int count, size_t stride, int p)
{
    float g = 0.0f;
    for (int r = 0; r < count; ++r) g += src[r * stride + p];
    return g;
}

// One thread: the four loss sums added in row order, then losses, mean(delta) and the gradient scales from N, the call's
// verdict into the sticky refusal count (a KL stop, bit 8 alone, is not a refusal and is not counted), the step counters.  The closed update (n_given >= 1) passes the workgroup
// partials with N = n_given and reads the verdict the gradient kernel left in the status word; the apply (n_given == 0)
// passes gradient rows, takes N and the verdict from their tails and writes the verdict to the status word.
__global__ void learner_finalize_kernel(const float *src, int count, size_t stride, int P, int64_t n_given, int per_sample,
                                        int *status, int *errors, int64_t *steps, float *scal, float *actor_loss,
                                        float *critic_loss)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int64_t N = n_given;
    int bad = 0;
    for (int r = 0; r < count; ++r) {
        const float *row = src + r * stride;
        for (int q = 0; q < 4; ++q) sum[q] += row[P + q];
        if (n_given) continue;                                      // a workgroup partial ends here
        const int32_t *tail = reinterpret_cast<const int32_t *>(row) + P + 4;
        const int64_t nr = (int64_t)((uint64_t)(uint32_t)tail[0] | ((uint64_t)(uint32_t)tail[1] << 32));
        bad |= tail[2] & (31 | 64 | 128);
        if (tail[3] != P || nr < 1) bad |= 32;                      // a row of another layout (or not a row at all)
        else N += nr;
    }
    if (n_given) bad = *status;
    else *status = bad;
    const float inv_n = 1.0f / (float)N;
    const float mean_nlp = sum[0] * inv_n, mean_delta = sum[1] * inv_n;
    const float al = per_sample ? sum[2] * inv_n : mean_nlp * mean_delta;
    const float cl = sum[3] * inv_n;
    if (actor_loss) *actor_loss = bad ? NAN : al;
    if (critic_loss) *critic_loss = bad ? NAN : cl;
    // gradient scales of the Adam kernel: actor, critic
    scal[0] = per_sample ? -inv_n : -mean_delta * inv_n;
    scal[1] = 2.0f * inv_n;
    if (bad & ~kLearnerStopped) *errors += 1;                       // a stop alone is not a refusal
    if (bad) return;
    for (int q = 0; q < kLearnerTensors; ++q) steps[q] += 1;
}

// Both torch.optim.Adam steps (adam_element, adam.h) on the gradient sums of `count` rows, added in row order and
// scaled once.
__global__ void learner_adam_kernel(float *params, float *m, float *v, const float *src, int count, size_t stride,
                                    LearnerLayout L, const int *status, const int64_t *steps, const float *scal,
                                    float actor_lr, float critic_lr)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= L.P || *status) return;
    const bool actor = p < L.c_w1;
    const float g = ordered_sum(src, count, stride, p) * (actor ? scal[0] : scal[1]);
    adam_element(params[p], m[p], v[p], g, steps[L.tensor_of(p)], actor ? actor_lr : critic_lr);
}

// The target critic's sync rule (uavtrack_learner_set_target), behind the Adam kernel of a closed update or an apply and
// gated on the same status word: one thread per word of the critic's block.  Polyak (period == 0):
// t <- fl(fl(omt * t) + fl(tau * w)), each operation rounded on its own (no contraction), tau and omt = 1.0f - tau formed
// on the host.  Periodic (period >= 1): t <- w when the critic's fc1.weight step count, which the finalize kernel has
// already advanced, is a multiple of period.  A refused update leaves the block alone.
__global__ void learner_target_kernel(float *target, const float *critic, int words, const int *status,
                                      const int64_t *steps, float tau, float omt, int64_t period)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= words || *status) return;
    if (period == 0) target[p] = __fadd_rn(__fmul_rn(omt, target[p]), __fmul_rn(tau, critic[p]));
    else if (steps[4] % period == 0) target[p] = critic[p];
}

// ---- gradient-norm clipping (torch.nn.utils.clip_grad_norm_, one max_norm per network), between "scale" and "Adam".
// Every sum has a fixed order -- ordered_sum per word, a fixed tree over the 256 words of a workgroup, workgroups
// ascending -- and is carried in fp64, so whoever clips the same rows in the same order gets the same coefficient bits.

constexpr int kClipThreads = 256;   // words per workgroup of learner_gradsum_kernel (= the Adam kernel's)

// One thread per word: g_p = ordered_sum * scal[network], the gradient the Adam kernel would form, into gsum[p]; the
// workgroup's two sums of g^2 (a workgroup may straddle the actor / critic boundary) into sq[workgroup][2].
__global__ void __launch_bounds__(kClipThreads) learner_gradsum_kernel(const float *src, int count, size_t stride,
                                                                       LearnerLayout L, const int *status,
                                                                       const float *scal, float *gsum, double *sq)
{
    __shared__ double part[2][kClipThreads];
    if (*status) return;                                            // uniform: a refused update forms no norm
    const int tid = threadIdx.x, p = blockIdx.x * kClipThreads + tid;
    double qa = 0.0, qc = 0.0;
    if (p < L.P) {
        const bool actor = p < L.c_w1;
        const float g = ordered_sum(src, count, stride, p) * (actor ? scal[0] : scal[1]);
        gsum[p] = g;
        const double q = (double)g * (double)g;
        if (actor) qa = q; else qc = q;
    }
    part[0][tid] = qa;
    part[1][tid] = qc;
    __syncthreads();
    for (int h = kClipThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            part[0][tid] += part[0][tid + h];
            part[1][tid] += part[1][tid + h];
        }
        __syncthreads();
    }
    if (tid == 0) {
        sq[2 * blockIdx.x + 0] = part[0][0];
        sq[2 * blockIdx.x + 1] = part[1][0];
    }
}

// One thread: the workgroups' sums of squares added in workgroup order, the two norms, and per network
// coef = min(1, max_norm / (norm + 1e-6)) formed in double and rounded to fp32 once (norm + 1e-6 <= max_norm gives
// exactly 1.0f; max_norm = +inf is "off": exactly 1.0f).  A NaN ratio stays NaN, as torch's clamp leaves it.
// grad_norm (nullable [2]): the two norms before clipping, NaN for a refused update.
__global__ void learner_clip_kernel(const double *sq, int groups, double actor_max, double critic_max, const int *status,
                                    float *coef, float *grad_norm)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (*status) {
        if (grad_norm) { grad_norm[0] = NAN; grad_norm[1] = NAN; }
        return;
    }
    double s[2] = {0.0, 0.0};
    for (int g = 0; g < groups; ++g) { s[0] += sq[2 * g]; s[1] += sq[2 * g + 1]; }
    const double mx[2] = {actor_max, critic_max};
    for (int k = 0; k < 2; ++k) {
        const double norm = sqrt(s[k]);
        const double r = mx[k] / (norm + 1e-6);
        coef[k] = isinf(mx[k]) || r >= 1.0 ? 1.0f : (float)r;
        if (grad_norm) grad_norm[k] = (float)norm;
    }
}

// ---- the split update (uavtrack_learner_grad / _apply / _write_priorities): the update cut between "sum" and "scale +
// Adam".  A gradient row is [P + kLearnerRowTail] words: the P gradient sums and the four loss sums, each the
// ordered_sum of the workgroup partials (what the closed update's Adam and finalize kernels form before they scale),
// then n (int64 as two words), the row's status bits and P as a layout tag.  The apply launches the same finalize and
// Adam kernels over rows instead of partials.  Every sum keeps a fixed order (workgroups ascending inside a row, rows
// ascending in the apply), so whoever applies the same rows in the same order gets the same bits, and one row gives the
// bits of the closed update (0.0f + x == x bitwise: a sum that starts from +0 is never -0).

// One thread per word of the row: the workgroup partials summed in workgroup order, then the tail.
__global__ void learner_reduce_kernel(const float *partials, int groups, int P, int64_t n, const int *status, float *row)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P + kLearnerRowTail) return;
    if (p < P + 4) {
        row[p] = ordered_sum(partials, groups, (size_t)P + 4, p);
        return;
    }
    int32_t *tail = reinterpret_cast<int32_t *>(row);
    const uint64_t un = (uint64_t)n;
    const int q = p - (P + 4);
    tail[p] = q == 0 ? (int32_t)(uint32_t)(un & 0xFFFFFFFFu) : q == 1 ? (int32_t)(uint32_t)(un >> 32) : q == 2 ? *status : P;
}

// the priorities: claim every sampled slot, keep the largest batch row per slot, mark it, write |delta| from it
__global__ void learner_prio_claim_kernel(const int64_t *idx, int64_t n, int64_t capacity, float *prio, const int *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || *status) return;
    const int64_t slot = idx ? idx[i] : i;
    if (slot >= 0 && slot < capacity) reinterpret_cast<int *>(prio)[slot] = -1;
}

__global__ void learner_prio_max_kernel(const int64_t *idx, int64_t n, int64_t capacity, float *prio, const int *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || *status) return;
    const int64_t slot = idx ? idx[i] : i;
    if (slot >= 0 && slot < capacity) atomicMax(reinterpret_cast<int *>(prio) + slot, (int)i);
}

__global__ void learner_prio_mark_kernel(const int64_t *idx, int64_t n, int64_t capacity, const float *prio,
                                         uint8_t *last, const int *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || *status) return;
    const int64_t slot = idx ? idx[i] : i;
    last[i] = (slot >= 0 && slot < capacity && reinterpret_cast<const int *>(prio)[slot] == (int)i) ? 1 : 0;
}

__global__ void learner_prio_write_kernel(const int64_t *idx, int64_t n, const float *td, float *prio,
                                          const uint8_t *last, const int *status)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || *status) return;
    if (last[i]) prio[idx ? idx[i] : i] = fabsf(td[i]);
}

// ---- the critic alone (uavtrack_learner_values): V(x) of n rows, the chain of learner_grad_kernel's V(s) to the bit.
// One lane owns two rows (i and i + kVW of the workgroup's chunk of 2 kVW): 24 inputs in registers from six 16-byte
// loads, consecutive lanes on consecutive 48-byte rows.  The critic's 14 H + 1 words are wavefront-uniform; the
// workgroup copies them into LDS once, one 64-byte record per hidden unit {W1c[j][0..11], b1c[j], W2c[j], -, -}, and
// every lane reads a record through the same address (four broadcast 16-byte LDS reads for 2 x 13 fused operations
// and two max).  The chains are explicit fmaf in the gradient kernel's order; nothing is reassociated.

constexpr int kVW = 256;          // threads per workgroup of the values kernel
constexpr int kVRec = 16;         // words per hidden unit's LDS record

__device__ __forceinline__ void load_row(float (&x)[12], const float *src)
{
    const float4 *s = reinterpret_cast<const float4 *>(src);
    const float4 a = s[0], b = s[1], c = s[2];
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    x[8] = c.x; x[9] = c.y; x[10] = c.z; x[11] = c.w;
}

// `critic` is a critic block [14 H + 1] in torch order: the online critic inside the parameter blob, or the target critic.
__global__ void __launch_bounds__(kVW) learner_values_kernel(const float *critic, int H, int64_t n,
                                                             const float *rows, float *values)
{
    __shared__ __attribute__((aligned(16))) float rec[kLearnerMaxHidden * kVRec];
    const int tid = threadIdx.x;
    const float *W1c = critic, *b1c = critic + 12 * H, *W2c = critic + 13 * H;
    for (int e = tid; e < H * kVRec; e += kVW) {
        const int j = e / kVRec, k = e - j * kVRec;
        rec[e] = k < 12 ? W1c[j * 12 + k] : (k == 12 ? b1c[j] : (k == 13 ? W2c[j] : 0.0f));
    }
    const float b2 = critic[14 * H];
    __syncthreads();
    const int64_t chunk = 2 * kVW;
    for (int64_t base = (int64_t)blockIdx.x * chunk; base < n; base += (int64_t)gridDim.x * chunk) {
        const int64_t i0 = base + tid, i1 = i0 + kVW;
        float x0[12], x1[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) { x0[k] = 0.0f; x1[k] = 0.0f; }
        if (i0 < n) load_row(x0, rows + i0 * 12);
        if (i1 < n) load_row(x1, rows + i1 * 12);
        float z0 = b2, z1 = b2;
#pragma unroll 2
        for (int j = 0; j < H; ++j) {
            const float4 *r = reinterpret_cast<const float4 *>(rec + j * kVRec);
            const float4 wa = r[0], wb = r[1], wc = r[2], tail = r[3];
            const float w[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
            float p0 = tail.x, p1 = tail.x;
#pragma unroll
            for (int k = 0; k < 12; ++k) {
                p0 = fmaf(w[k], x0[k], p0);
                p1 = fmaf(w[k], x1[k], p1);
            }
            z0 = fmaf(tail.y, fmaxf(p0, 0.0f), z0);
            z1 = fmaf(tail.y, fmaxf(p1, 0.0f), z1);
        }
        if (i0 < n) values[i0] = z0;
        if (i1 < n) values[i1] = z1;
    }
}

// ---- batch-normalised advantages (uavtrack_learner_set_advantage, UAVTRACK_ADVANTAGE_BATCH): delta of every row and its
// mean and standard deviation, ahead of the gradient kernel.  Rows are taken in chunks of kAdvChunk = 256 consecutive rows
// (chunk c is rows [256 c, 256 c + 256) whatever the grid is; rows past n count as 0.0 and are not counted in n).  A chunk's
// 256 fp64 terms are added by the fixed halving tree x[k] += x[k + h], h = 128 .. 1, and the chunk sums in ascending chunk
// order by one thread, so no sum depends on the launch geometry.

constexpr int kAdvChunk = 256;    // rows per chunk = threads per workgroup of the two kernels below

struct TdArgs {
    const float *critic;            // [14 H + 1] the online critic's block: V(s)
    const float *target;            // [14 H + 1] the block V(s') is formed from (the same pointer while no target critic is on)
    const float *states, *rewards, *next_states;
    const int64_t *idx;             // nullable: rows 0..n-1
    const float *discounts;         // nullable [capacity], slot order
    int64_t n, capacity;
    int H;
    float gamma;
    float *td;                      // [n] delta_i, 0 for a row whose index is out of range (the gradient kernel refuses it)
    double *psum;                   // [chunks] the chunks' sums of delta
};

__device__ __forceinline__ double chunk_tree(double *part, int tid, double x)
{
    part[tid] = x;
    __syncthreads();
    for (int h = kAdvChunk / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    const double s = part[0];
    __syncthreads();
    return s;
}

// delta_i = (r_i + d_i V'(s'_i)) - V(s_i), one lane per row: the layer-1 and layer-2 chains of the gradient kernel
// (explicit fmaf in k and j order, as learner_values_kernel has them) and the target as one multiply and one add, each
// rounded on its own, so td[i] holds the bits the gradient kernel forms for the row.  Both critic blocks wait in LDS as
// learner_values_kernel's records.
__global__ void __launch_bounds__(kAdvChunk) learner_td_kernel(TdArgs a)
{
    __shared__ __attribute__((aligned(16))) float rec[2][kLearnerMaxHidden * kVRec];
    __shared__ double part[kAdvChunk];
    const int tid = threadIdx.x, H = a.H;
    for (int b = 0; b < 2; ++b) {
        const float *blk = b ? a.target : a.critic;
        for (int e = tid; e < H * kVRec; e += kAdvChunk) {
            const int j = e / kVRec, k = e - j * kVRec;
            rec[b][e] = k < 12 ? blk[j * 12 + k] : (k == 12 ? blk[12 * H + j] : (k == 13 ? blk[13 * H + j] : 0.0f));
        }
    }
    const float b2 = a.critic[14 * H], b2t = a.target[14 * H];
    __syncthreads();
    const int64_t chunks = (a.n + kAdvChunk - 1) / kAdvChunk;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * kAdvChunk + tid;
        float delta = 0.0f;
        if (i < a.n) {
            const int64_t src = a.idx ? a.idx[i] : i;
            if (src >= 0 && src < a.capacity) {
                float x[12], y[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) { x[k] = a.states[src * 12 + k]; y[k] = a.next_states[src * 12 + k]; }
                float v = b2, vn = b2t;
                for (int j = 0; j < H; ++j) {
                    const float4 *r = reinterpret_cast<const float4 *>(rec[0] + j * kVRec);
                    const float4 *t = reinterpret_cast<const float4 *>(rec[1] + j * kVRec);
                    const float4 wa = r[0], wb = r[1], wc = r[2], wd = r[3];
                    const float4 ta = t[0], tb = t[1], tc = t[2], tdl = t[3];
                    const float w[12] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w, wc.x, wc.y, wc.z, wc.w};
                    const float u[12] = {ta.x, ta.y, ta.z, ta.w, tb.x, tb.y, tb.z, tb.w, tc.x, tc.y, tc.z, tc.w};
                    float p = wd.x, q = tdl.x;
#pragma unroll
                    for (int k = 0; k < 12; ++k) {
                        p = fmaf(w[k], x[k], p);
                        q = fmaf(u[k], y[k], q);
                    }
                    v = fmaf(wd.y, fmaxf(p, 0.0f), v);
                    vn = fmaf(tdl.y, fmaxf(q, 0.0f), vn);
                }
                const float d = a.discounts ? a.discounts[src] : a.gamma;
                const float target = __fadd_rn(a.rewards[src], __fmul_rn(d, vn));
                delta = __fsub_rn(target, v);
            }
            a.td[i] = delta;
        }
        const double s = chunk_tree(part, tid, (double)delta);
        if (tid == 0) a.psum[c] = s;
    }
}

// In learner_td_kernel's place when the batch brings stored advantages: td[i] = advantages[src_i], the value the
// gradient kernel will standardise (0 for a row whose index is out of range), and each chunk's fp64 sum by the same tree.
__global__ void __launch_bounds__(kAdvChunk) learner_adv_gather_kernel(const float *advantages, const int64_t *idx,
                                                                       int64_t n, int64_t capacity, float *td, double *psum)
{
    __shared__ double part[kAdvChunk];
    const int tid = threadIdx.x;
    const int64_t chunks = (n + kAdvChunk - 1) / kAdvChunk;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * kAdvChunk + tid;
        float x = 0.0f;
        if (i < n) {
            const int64_t src = idx ? idx[i] : i;
            if (src >= 0 && src < capacity) x = advantages[src];
            td[i] = x;
        }
        const double s = chunk_tree(part, tid, (double)x);
        if (tid == 0) psum[c] = s;
    }
}

// the chunk sums in ascending chunk order
__device__ __forceinline__ double ordered_sum64(const double *src, int64_t count)
{
    double s = 0.0;
    for (int64_t c = 0; c < count; ++c) s += src[c];
    return s;
}

// Q's chunk sums: (delta_i - mean64)^2 with the difference, the product and the adds as separate fp64 operations;
// mean64 = S / n, S formed by thread 0 of every workgroup in the one order
__global__ void __launch_bounds__(kAdvChunk) learner_adv_sq_kernel(const float *td, int64_t n, const double *psum, double *psq)
{
    __shared__ double part[kAdvChunk];
    __shared__ double mean_s;
    const int tid = threadIdx.x;
    const int64_t chunks = (n + kAdvChunk - 1) / kAdvChunk;
    if (tid == 0) mean_s = __ddiv_rn(ordered_sum64(psum, chunks), (double)n);
    __syncthreads();
    const double mean = mean_s;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * kAdvChunk + tid;
        double q = 0.0;
        if (i < n) {
            const double d = __dsub_rn((double)td[i], mean);
            q = __dmul_rn(d, d);
        }
        const double s = chunk_tree(part, tid, q);
        if (tid == 0) psq[c] = s;
    }
}

// One thread: stats = {(float)mean64, (float)inv64, (float)std64}, std64 = sqrt(Q / (n - 1)) (the unbiased form, n >= 2),
// inv64 = 1 / (std64 + eps)
__global__ void learner_adv_stats_kernel(const double *psum, const double *psq, int64_t n, double eps, float *stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int64_t chunks = (n + kAdvChunk - 1) / kAdvChunk;
    const double mean = __ddiv_rn(ordered_sum64(psum, chunks), (double)n);
    const double var = __ddiv_rn(ordered_sum64(psq, chunks), (double)(n - 1));
    const double sd = __dsqrt_rn(var);
    const double inv = __ddiv_rn(1.0, __dadd_rn(sd, eps));
    stats[0] = (float)mean; stats[1] = (float)inv; stats[2] = (float)sd;
}

// behind the gradient kernel: the statistics of a refused update are NaN
__global__ void learner_adv_seal_kernel(const int *status, float *stats)
{
    if (threadIdx.x != 0 || blockIdx.x != 0 || !*status) return;
    stats[0] = NAN; stats[1] = NAN; stats[2] = NAN;
}

// ---- KL early stopping (uavtrack_learner_set_kl_stop): behind the gradient kernel of a closed clipped update, ahead of
// the finalize kernel (batch mode's seal moves behind this pass, so a stopped update's statistics are NaN too).  k_i = (r_i - 1) - log r_i of the fp32 ratio the gradient kernel left for batch row
// i, widened to fp64 (two subtractions and a log: r == 1 gives exactly 0, r == 0 gives +inf), summed in the order of the
// advantage statistics: chunks of 256 rows, the halving tree, chunk sums ascending.  A refused update (its ratios hold
// NaN) and a latched one (the gradient kernel wrote none) form no sum.

__global__ void __launch_bounds__(kAdvChunk) learner_kl_chunk_kernel(const float *ratio, int64_t n, const int *status,
                                                                     double *part)
{
    __shared__ double sh[kAdvChunk];
    if (*status) return;                                            // uniform
    const int tid = threadIdx.x;
    const int64_t chunks = (n + kAdvChunk - 1) / kAdvChunk;
    for (int64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const int64_t i = c * kAdvChunk + tid;
        double k = 0.0;
        if (i < n) {
            const double r = (double)ratio[i];
            k = __dsub_rn(__dsub_rn(r, 1.0), log(r));
        }
        const double s = chunk_tree(sh, tid, k);
        if (tid == 0) part[c] = s;
    }
}

// One thread: kl = (float)(sum / n); where kl > limit in fp32 the latch is set and the update stopped (status bit 8), so
// everything behind this kernel that is gated on the status word skips it.  state = {stopped, skipped}: an update that
// trips the latch or meets it set counts as skipped.  kl_out keeps the last evaluated batch's value under a latched
// update and is NaN for a refused one, which never sets the latch.
__global__ void learner_kl_kernel(const double *part, int64_t n, float limit, int *status, float *kl_out, int32_t *state)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int st = *status;
    if (st & kLearnerStopped) { state[1] += 1; return; }
    if (st) { *kl_out = NAN; return; }
    const float kl = (float)__ddiv_rn(ordered_sum64(part, (n + kAdvChunk - 1) / kAdvChunk), (double)n);
    *kl_out = kl;
    if (kl > limit) {
        state[0] = 1;
        state[1] += 1;
        *status = kLearnerStopped;
    }
}

__global__ void learner_kl_reset_kernel(int32_t *state)
{
    if (threadIdx.x == 0 && blockIdx.x == 0) { state[0] = 0; state[1] = 0; }
}

}  // namespace

int64_t learner_adv_chunks(int64_t n) { return (n + kAdvChunk - 1) / kAdvChunk; }

hipError_t launch_learner_values(const LearnerDevice &d, bool target, int64_t n, const float *rows, float *values,
                                 hipStream_t st)
{
    static_assert(kLearnerMaxHidden * kVRec * sizeof(float) <= 64 * 1024, "the critic's records fit static LDS");
    int64_t blocks = (n + 2 * kVW - 1) / (2 * kVW);
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(learner_values_kernel, dim3((unsigned)blocks), dim3(kVW), 0, st,
                       target ? d.target : d.params + d.L.c_w1, d.L.H, n, rows, values);
    return hipGetLastError();
}

int learner_rows_per_tile(int hidden)
{
    const int r = 4096 / (hidden < 16 ? 16 : hidden);
    return r > 256 ? 256 : r;
}

size_t learner_lds_bytes(const LearnerLayout &L, int rows, int extra_floats_per_row)
{
    return sizeof(float) * ((size_t)L.P + (size_t)rows * (24 + 3 * L.H + L.A + 2 + 4 + 2 + extra_floats_per_row)) +
           sizeof(int) * (size_t)rows;
}

int learner_groups(const LearnerLayout &L, int64_t n)
{
    const int64_t R = learner_rows_per_tile(L.H);
    const int64_t tiles = (n + R - 1) / R;
    return (int)(tiles < kLearnerMaxGroups ? tiles : kLearnerMaxGroups);
}

int learner_clip_groups(const LearnerLayout &L) { return (L.P + kClipThreads - 1) / kClipThreads; }

namespace {

// learner_variants.h's table over the kernels themselves, in its order
#define GRAD_KERNEL_ROW(k, reg, tgt, clip, adv, stored, lds) k,
void (*const kGradKernels[kLearnerGradVariantCount])(GradArgs) = {UAVTRACK_LEARNER_GRAD_VARIANTS(GRAD_KERNEL_ROW)};
#undef GRAD_KERNEL_ROW

}  // namespace

hipError_t learner_prepare_kernels(const LearnerLayout &L)
{
    // every instantiation of the gradient body needs the attribute of its own: up to about 131 KB at H = 256
    const int R = learner_rows_per_tile(L.H);
    for (int i = 0; i < kLearnerGradVariantCount; ++i) {
        const size_t lds = learner_lds_bytes(L, R, kLearnerGradVariants[i].lds_extra);
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kGradKernels[i]),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

namespace {

hipError_t launch_grad(const LearnerDevice &d, const LearnerLaunch &q, float *td, int *status, hipStream_t st)
{
    const LearnerLayout &L = d.L;
    const int R = learner_rows_per_tile(L.H);
    // KL early stopping (closed clipped updates only; the host has refused every other form while it is on)
    if (d.kl_on) hipLaunchKernelGGL(learner_begin_kl_kernel, dim3(1), dim3(64), 0, st, status, d.kl_state);
    else hipLaunchKernelGGL(learner_begin_kernel, dim3(1), dim3(64), 0, st, status);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;

    const bool batch = d.adv_mode == kAdvantageBatch, stored = q.advantages != nullptr;
    GradArgs a;
    a.params = d.params; a.states = q.states; a.rewards = q.rewards; a.next_states = q.next_states;
    a.actions = q.actions; a.idx = q.idx; a.weights = q.weights; a.n = q.n; a.capacity = q.capacity;
    a.partials = d.partials; a.td_delta = td; a.status = status;
    a.L = L; a.rows = R; a.gamma = d.gamma; a.per_sample = d.per_sample;
    a.entropy_coef = d.entropy_coef; a.entropy = d.entropy; a.discounts = q.discounts;
    a.target = d.target_mode ? d.target : nullptr;
    a.log_mu = q.log_mu; a.clip_lo = q.clip_lo; a.clip_hi = q.clip_hi; a.ratio = q.ratio;
    a.stats = batch ? d.stats() : d.adv_given;
    a.advantages = q.advantages;
    a.latch = d.kl_on ? d.kl_state : nullptr;
    if (d.kl_on && !a.ratio) a.ratio = d.kl_ratio;                  // the KL pass reads the ratios: the handle's scratch
    // a stored advantage passes through the normalised advantage's line in every mode: raw is the constant pair {0, 1}
    if (stored && d.adv_mode == kAdvantageRaw) a.stats = d.adv_unit;
    const int variant = learner_grad_variant(d.entropy_coef != 0.0f || d.entropy, a.target != nullptr, q.log_mu != nullptr,
                                             d.adv_mode != kAdvantageRaw, stored);
    if (batch) {
        // the normalised advantage in batch mode: the TD pass (stored advantages: their gather) and the statistics
        // first, the seal behind
        const int64_t chunks = learner_adv_chunks(q.n);
        const dim3 cgrid((unsigned)(chunks < 1024 ? chunks : 1024));
        double *psum = d.adv_part, *psq = d.adv_part + learner_adv_chunks(d.max_n);
        if (stored) {
            hipLaunchKernelGGL(learner_adv_gather_kernel, cgrid, dim3(kAdvChunk), 0, st, q.advantages, q.idx, q.n,
                               q.capacity, d.adv_td, psum);
        } else {
            TdArgs t;
            t.critic = d.params + L.c_w1; t.target = a.target ? a.target : t.critic;
            t.states = q.states; t.rewards = q.rewards; t.next_states = q.next_states; t.idx = q.idx;
            t.discounts = q.discounts; t.n = q.n; t.capacity = q.capacity; t.H = L.H; t.gamma = d.gamma;
            t.td = d.adv_td; t.psum = psum;
            hipLaunchKernelGGL(learner_td_kernel, cgrid, dim3(kAdvChunk), 0, st, t);
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(learner_adv_sq_kernel, cgrid, dim3(kAdvChunk), 0, st, d.adv_td, q.n, psum, psq);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(learner_adv_stats_kernel, dim3(1), dim3(64), 0, st, psum, psq, q.n, d.adv_eps, d.stats());
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    const dim3 grid(learner_groups(L, q.n));
    hipLaunchKernelGGL(kGradKernels[variant], grid, dim3(kLW), learner_lds_bytes(L, R, kLearnerGradVariants[variant].lds_extra),
                       st, a);
    if ((e = hipGetLastError()) != hipSuccess || !batch || d.kl_on) return e;   // (the KL pass's verdict first: the seal follows it)
    hipLaunchKernelGGL(learner_adv_seal_kernel, dim3(1), dim3(64), 0, st, status, d.stats());
    return hipGetLastError();
}

// The tail both forms share: finalize over `count` rows of `stride` words (n_given as learner_finalize_kernel takes
// it), then Adam over the same rows.
hipError_t launch_scale_adam(const LearnerDevice &d, const float *src, int count, size_t stride, int64_t n_given,
                             float *actor_loss, float *critic_loss, hipStream_t st)
{
    const LearnerLayout &L = d.L;
    hipLaunchKernelGGL(learner_finalize_kernel, dim3(1), dim3(64), 0, st, src, count, stride, L.P, n_given, d.per_sample,
                       d.opt.status, d.opt.errors, d.opt.steps, d.scal, actor_loss, critic_loss);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const float *scal = d.scal;
    if (std::isfinite(d.max_norm[0]) || std::isfinite(d.max_norm[1])) {
        // the clip: the scaled gradient once into gsum, its norms, then Adam over (gsum, one row, the coefficients).
        // 0.0f + g == g for the moments and the parameters: where g is -0 the sum is +0, and adam_element gives the
        // same m, v and w from either zero.
        const int groups = learner_clip_groups(L);
        hipLaunchKernelGGL(learner_gradsum_kernel, dim3(groups), dim3(kClipThreads), 0, st, src, count, stride, L,
                           d.opt.status, d.scal, d.gsum, d.sq);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(learner_clip_kernel, dim3(1), dim3(64), 0, st, d.sq, groups, d.max_norm[0], d.max_norm[1],
                           d.opt.status, d.coef, d.grad_norm);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        src = d.gsum; count = 1; stride = (size_t)L.P; scal = d.coef;
    }
    hipLaunchKernelGGL(learner_adam_kernel, dim3((L.P + 255) / 256), dim3(256), 0, st, d.params, d.opt.m, d.opt.v, src,
                       count, stride, L, d.opt.status, d.opt.steps, scal, d.actor_lr, d.critic_lr);
    if ((e = hipGetLastError()) != hipSuccess || !d.target_mode) return e;
    // the target critic's sync rule, once per successful update or apply (period 0: Polyak)
    const int words = learner_critic_words(L);
    hipLaunchKernelGGL(learner_target_kernel, dim3((words + 255) / 256), dim3(256), 0, st, d.target, d.params + L.c_w1,
                       words, d.opt.status, d.opt.steps, d.target_tau, d.target_omt, d.target_period);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_learner_priorities(const LearnerDevice &d, const int64_t *idx, int64_t n, int64_t capacity,
                                     const float *td, float *prio, hipStream_t st)
{
    const dim3 grid((unsigned)((n + 255) / 256)), blk(256);
    hipError_t e;
    hipLaunchKernelGGL(learner_prio_claim_kernel, grid, blk, 0, st, idx, n, capacity, prio, d.opt.status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(learner_prio_max_kernel, grid, blk, 0, st, idx, n, capacity, prio, d.opt.status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(learner_prio_mark_kernel, grid, blk, 0, st, idx, n, capacity, prio, d.last, d.opt.status);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(learner_prio_write_kernel, grid, blk, 0, st, idx, n, td, prio, d.last, d.opt.status);
    return hipGetLastError();
}

hipError_t launch_learner_kl_reset(const LearnerDevice &d, hipStream_t st)
{
    hipLaunchKernelGGL(learner_kl_reset_kernel, dim3(1), dim3(64), 0, st, d.kl_state);
    return hipGetLastError();
}

hipError_t launch_learner_update(const LearnerDevice &d, const LearnerLaunch &q, hipStream_t st)
{
    float *td = q.td_delta ? q.td_delta : d.td;
    hipError_t e = launch_grad(d, q, td, d.opt.status, st);
    if (e != hipSuccess) return e;
    if (d.kl_on) {
        // the minibatch's own KL estimate from the ratios of the policy as it stands, and the verdict, ahead of the step
        const int64_t chunks = learner_adv_chunks(q.n);
        hipLaunchKernelGGL(learner_kl_chunk_kernel, dim3((unsigned)(chunks < 1024 ? chunks : 1024)), dim3(kAdvChunk), 0, st,
                           q.ratio ? q.ratio : d.kl_ratio, q.n, d.opt.status, d.kl_part);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(learner_kl_kernel, dim3(1), dim3(64), 0, st, d.kl_part, q.n, d.kl_limit, d.opt.status, d.kl_out,
                           d.kl_state);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (d.adv_mode == kAdvantageBatch) {
            // batch-mode statistics of a stopped update are NaN like a refused one's: the seal behind the verdict
            hipLaunchKernelGGL(learner_adv_seal_kernel, dim3(1), dim3(64), 0, st, d.opt.status, d.stats());
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    e = launch_scale_adam(d, d.partials, learner_groups(d.L, q.n), (size_t)d.L.P + 4, q.n, q.actor_loss, q.critic_loss, st);
    if (e != hipSuccess) return e;
    if (q.priorities) return launch_learner_priorities(d, q.idx, q.n, q.capacity, td, q.priorities, st);
    return hipSuccess;
}

// The gradient half of the split update: q.td_delta is required, q.actor_loss / critic_loss / priorities are not used.
// The bad-input bits go to the handle's grad status word, so the verdict of the last apply stays in opt.status.
hipError_t launch_learner_grad(const LearnerDevice &d, const LearnerLaunch &q, float *row, hipStream_t st)
{
    const int P = d.L.P;
    hipError_t e = launch_grad(d, q, q.td_delta, d.gstatus, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(learner_reduce_kernel, dim3((P + kLearnerRowTail + 255) / 256), dim3(256), 0, st, d.partials,
                       learner_groups(d.L, q.n), P, q.n, d.gstatus, row);
    return hipGetLastError();
}

hipError_t launch_learner_apply(const LearnerDevice &d, const float *rows, int count, float *actor_loss,
                                float *critic_loss, hipStream_t st)
{
    return launch_scale_adam(d, rows, count, (size_t)d.L.P + kLearnerRowTail, 0, actor_loss, critic_loss, st);
}

}  // namespace uavtrack

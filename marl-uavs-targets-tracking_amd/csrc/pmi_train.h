// pmi_train.h -- the device PMI trainer (uavtrack_pmi_trainer_*): what pmi_train_kernel.hip and api_pmi_trainer.hip share.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "adam.h"
#include "pmi_net.h"

namespace uavtrack {

// pmi_train_kernel.hip -- the device PMI trainer (uavtrack_pmi_trainer_*).  `state` holds the float entries of the
// reference PMINetwork's state_dict in its order (26 tensors: per Linear+BatchNorm1d block weight, bias, bn weight, bn
// bias, running_mean, running_var; then fc2.weight, fc2.bias); the gradients and Adam moments hold the 18 trainable
// tensors in PMINetwork.parameters() order (per block weight, bias, bn weight, bn bias; then fc2).
constexpr int64_t kPmiTrainMaxBatch = (int64_t)1 << 20;
struct PmiTrainLayout {
    int H, S, P;
    int soff[kPmiStateTensors + 1];           // state tensor offsets (soff[26] = S)
    int poff[kPmiTrainTensors + 1];           // trainable tensor offsets (poff[18] = P)
    __host__ __device__ static int state_of(int t) { return t < 16 ? (t / 4) * 6 + t % 4 : t + 8; }
    static PmiTrainLayout make(int H)
    {
        PmiTrainLayout L;
        L.H = H;
        const int in[kPmiBlocks] = {5, 4, 3, 3 * H};
        int ssz[kPmiStateTensors], k = 0;
        for (int b = 0; b < kPmiBlocks; ++b) {
            ssz[k++] = H * in[b];
            for (int q = 0; q < 5; ++q) ssz[k++] = H;
        }
        ssz[k++] = H;
        ssz[k++] = 1;
        L.soff[0] = 0;
        for (int t = 0; t < kPmiStateTensors; ++t) L.soff[t + 1] = L.soff[t] + ssz[t];
        L.poff[0] = 0;
        for (int t = 0; t < kPmiTrainTensors; ++t) L.poff[t + 1] = L.poff[t] + ssz[state_of(t)];
        L.S = L.soff[kPmiStateTensors];
        L.P = L.poff[kPmiTrainTensors];
        return L;
    }
};
// the device state of one trainer handle
struct PmiTrainDevice {
    PmiTrainLayout L;
    float lr;
    float *state;                   // [S] state_dict floats
    int64_t *nbt;                   // [4] num_batches_tracked per BatchNorm1d
    float *grad;                    // [P]
    AdamState opt;                  // kPmiTrainTensors tensors over [P]
    // per-step scratch, feature-major ([side][feature][row]) for batches up to max_b rows
    float *xh0, *a0, *da0;          // [2][3H][max_b] branch BN: normalised input, post-ReLU output, dL/d(output)
    float *xh1, *a1, *dz1;          // [2][H][max_b]  bn1: normalised input, post-ReLU output; dL/d(fc1 output)
    float *inv0, *inv1;             // [2][3H], [2][H] 1 / sqrt(var + eps) of the current step
    float *go;                      // [2][max_b] dL/d(output_1_2), dL/d(output_1_3)
    float *acc;                     // [1] sum of |loss| over the call
    // uavtrack_pmi_trainer_train_many: the selected rows of up to max_b draws and the identity triples that address them
    float *sel;                     // [max_b][2][12]
    int64_t *sel_t, *sel_u;         // [max_b] = i, [max_b][2] = (0, 1)
    int64_t max_b;
};
struct PmiTrainLaunch {
    const float *rows;
    int64_t n_rows, n_uav, b2, batch;
    const int64_t *t_idx, *u_idx;
    float *avg_loss, *losses, *outputs;
};
hipError_t launch_pmi_train(const PmiTrainDevice &d, const PmiTrainLaunch &q, hipStream_t stream);
// A source list as the select kernel takes it, by value: source k holds the timeline's groups [base[k], base[k + 1])
constexpr int kPmiMaxSources = 64;            // UAVTRACK_PMI_MAX_SOURCES
struct PmiSourceTable {
    const float *rows[kPmiMaxSources];
    int64_t base[kPmiMaxSources + 1];         // base[0]: the span's first group in the timeline
    int count;
};
// uavtrack_pmi_trainer_train_many: q.rows is unused, q.n_rows = total groups * n_uav
hipError_t launch_pmi_train_many(const PmiTrainDevice &d, const PmiSourceTable &src, const PmiTrainLaunch &q,
                                 hipStream_t stream);
// uavtrack_pmi_trainer_select: the draws of the table's span into selected [b2][2][12]
hipError_t launch_pmi_select(const PmiTrainDevice &d, const PmiSourceTable &src, int64_t total_groups, int64_t n_uav,
                             const int64_t *t_idx, const int64_t *u_idx, int64_t b2, float *selected, hipStream_t stream);

}  // namespace uavtrack

// pmi_net.h -- the shape of a PMINetwork that the scorer, the device pack and the trainer all need.
#pragma once

namespace uavtrack {

constexpr int kPmiTrainTensors = 18;
constexpr int kPmiStateTensors = 26;
constexpr int kPmiBlocks = 4;                 // fc_comm, fc_obs, fc_boundary_state, fc1 (each with a BatchNorm1d)
constexpr int kPmiMaxHidden = 256;                  // widest PMINetwork hidden layer the scorer is instantiated for

}  // namespace uavtrack

// ms_env_auct_launch.h — the launchers of env_auct_kernels.hip as capi.cpp calls them: the fixed-price fused
// launches (ms_env_launch.h's launch_env_step_act / launch_env_rollout_act) with a learned auctioneer, a third net
// that acts for the cores nobody owns.
#pragma once

#include <hip/hip_runtime.h>

#include "ms_layout.h"

namespace ms {

// the auctioneer's next-round acting (env_auct_kernels.hip auct_act): one net shared by the C cores, item
// e * C + c; the seed, the device offset and the common row are the FusedAct's beside it
struct AuctAct {
    ms_mlp_params net;  // the acceptor's shape; act fragments with the common row's table
    uint64_t offset;
    int8_t* action;  // [E][C]
    float* logprob;  // [E][C]
};

// the rounds of one launch_env_rollout_act_auct: RoundStride's strides and the auctioneer's own (bytes per round)
struct AuctRollout {
    RoundStride st;
    int64_t act_auct;                  // StepIO::act_auct
    int64_t auct_action, auct_logprob;  // AuctAct's outputs
    int n_rounds, act_last;
};

// one round with io.act_auct as the auctioneer's actions, then the next round's acting of the three nets
hipError_t launch_env_step_act_auct(const EnvDev& d, const StepIO& io, const FusedAct& fa, const AuctAct& aa,
                                    hipStream_t s);
// ro.n_rounds of launch_env_step_act_auct in one launch, round t's arrays ro's strides past round 0's
hipError_t launch_env_rollout_act_auct(const EnvDev& d, const StepIO& io, const FusedAct& fa, const AuctAct& aa,
                                       const AuctRollout& ro, hipStream_t s);

}  // namespace ms

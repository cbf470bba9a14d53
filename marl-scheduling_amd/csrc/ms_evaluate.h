// ms_evaluate.h — launch arguments and launcher of the policy evaluation kernel (evaluate_kernels.hip), shared
// with capi.cpp, which fills the struct field by field; the kernel takes it as it is. No device code here.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/marlsched.h"

namespace ms {

// k_evaluate (ActorCritic.evaluate: the log-prob of a given action, the state value, the entropy)
struct EvalArgs {
    ms_mlp_params actor, critic;  // critic used only with value != NULL
    const int8_t* obs;            // [E][U][stride]
    const int8_t* actions;        // [E][U] or NULL (logprob == NULL)
    int stride, U, S;
    int E, n_items;
    int tiles_per_wave, waves_per_group;
    float* logprob;  // [E][U] each, or NULL: neither written nor computed
    float* value;
    float* entropy;
};

// The launcher sets the wave split (tiles_per_wave, waves_per_group), the caller the rest. One launch of
// k_evaluate; InvalidValue: a shape the kernel is not built for, nothing launched (evaluate_kernels.hip)
hipError_t dispatch_evaluate(EvalArgs& a, hipStream_t st);

}  // namespace ms

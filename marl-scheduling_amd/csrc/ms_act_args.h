// ms_act_args.h — launch arguments and launchers of the acting kernels (policy_kernels.hip, act_pair_kernels.hip,
// greedy_kernels.hip), shared with capi.cpp, which fills the structs field by field; the kernels take them as they
// are. No device code here (the kernels' bodies and the units' launch plumbing: ms_act_kernels.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/marlsched.h"

namespace ms {

// k_act / k_act_common / k_act_pair (sampling)
struct ActArgs {
    ms_mlp_params n1, n2;  // n2 used only with a price net (NT2 > 0)
    const int8_t* obs;
    int stride, U, S, n_cores;
    int E, n_items;
    int tiles_per_wave, waves_per_group;
    uint64_t seed, offset;
    const uint64_t* offset_dev;
    const float* uniforms;  // [2][E*U] or NULL
    int8_t* action;
    float* logprob;
    int8_t* price_state;   // [E*U][4] (pus = 0) or unit-major: row (e, u) at u * pus + e
    int8_t* price_action;
    float* price_logprob;
    int64_t pus;           // unit stride (rows) of the price chooser's outputs; 0: [E][U]
    int8_t* env_price;
    const int8_t* common;  // [stride] or NULL (k_act_common)
    int items_per_wave;    // k_act_common
    // compact acceptor observations (k_act_common<.., OWN>): obs = core rows [E][C][stride], owner
    // [E][C]; row (e, u = a*C + c) is core row (e, c) if owner[e][c] == a + 1, else the common row
    const int8_t* owner;
    // price chooser sampling table (ms_price_table): ptab [G][pkeys][kPriceTW], pdigit [4][256]
    // (key offset of byte value v at position p, index v + 128; -1: not tabulated); NULL: computed
    const float* ptab;
    const int16_t* pdigit;
    int pkeys;
};

// k_greedy / k_greedy_common / k_greedy_pair (argmax)
struct GreedyArgs {
    ms_mlp_params n1, n2;  // n2: the price chooser (NT2 > 0 only)
    const int8_t* obs;     // [E][U][stride], or with owner the core rows [E][C][stride]
    const int8_t* owner;   // [E][C] or NULL: row (e, u = a*C + c) is core row (e, c) if owner[e][c] == a + 1
    const int8_t* common;  // [stride] or NULL
    int stride, U, S, n_cores;
    int E, n_items;
    int tiles_per_wave, items_per_wave, waves_per_group;
    int8_t* action;
    float* logprob;        // or NULL
    int8_t* price_state;   // [E*U][4]
    int8_t* price_action;
    int8_t* env_price;
};

// The launchers set the wave split (tiles_per_wave, items_per_wave, waves_per_group), the caller the rest;
// n2.n_groups > 0: a price net beside the core chooser (a free-price round's offer units).
// one launch of k_act or k_act_common, whichever a's shape and common row ask for (policy_kernels.hip)
hipError_t dispatch_act(ActArgs& a, hipStream_t st);
// both halves of a round's acting (offer units; acceptors on compact rows) in one launch where their shapes have a
// paired kernel, else the two launches in order; Philox draws only (act_pair_kernels.hip)
hipError_t launch_act_round(ActArgs& offer, ActArgs& acceptor, hipStream_t st);
// one launch of k_greedy or k_greedy_common; InvalidValue: a shape the kernels are not built for (greedy_kernels.hip)
hipError_t dispatch_greedy(GreedyArgs& a, hipStream_t st);
// launch_act_round with both halves greedy (greedy_kernels.hip)
hipError_t launch_act_round_greedy(GreedyArgs& offer, GreedyArgs& acceptor, hipStream_t st);
// the price chooser's sampling table of K tabulated 4-byte inputs per group (policy_kernels.hip)
hipError_t launch_price_table(const ms_mlp_params* pn, const int8_t* rows, int K, float* tab, hipStream_t st);
// bytes of a net's act fragment block for rows of that stride, 0: shape not built (policy_kernels.hip)
size_t act_frag_bytes(const ms_mlp_params* p, int stride);
// the weights as the acting waves hold them and, with a common row, its sampling table (policy_kernels.hip)
hipError_t launch_act_prepare(const ms_mlp_params* p, const int8_t* common, int stride, void* frag, hipStream_t st);

}  // namespace ms

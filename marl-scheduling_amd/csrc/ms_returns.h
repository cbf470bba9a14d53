// ms_returns.h — the launchers of the rollout post-processing units, shared with capi.cpp: returns_kernels.hip
// (discounted, normalised returns) and agg_kernels.hip (aggregated observations and actions, regenerated agent rows;
// their AggArgs and RegenArgs are in ms_layout.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ms_layout.h"

namespace ms {

// ---- returns_kernels.hip
// the returns of sequence (e, g) = unit unit_of_group[g] of replica e from the rollout rewards [T][E][U] (f32, or
// int32 with is_i32), written time-major: out [T][E][G]
struct UnitReturns {
    const void* rewards;
    int is_i32, T, U, G;
    int64_t E;
    const int32_t* unit_of_group;  // [G]
    double gamma;
    float* out;
};
hipError_t launch_unit_returns(const UnitReturns& a, hipStream_t st);
// the same of M sequences given as rewards [T][row_stride] (sequence m in column m), out [M][T]
hipError_t launch_returns(const float* rewards, int T, int64_t M, int64_t row_stride, double gamma, float* out,
                          hipStream_t st);

// ---- agg_kernels.hip
// divided observation rows into the aggregated and fully aggregated agents' rows
hipError_t launch_aggregate_obs(const AggArgs& g, hipStream_t st);
// aggregated action numbers [EN] (fully: one per agent; else acceptor numbers, then offer numbers) into divided
// acceptor [EN][C] and offer [EN][L] actions; *bad (device, may be NULL) counts numbers out of range
struct DecodeArgs {
    const int32_t* actions;
    long long EN;  // replicas * agents
    int C, L, O, fully;
    int8_t *acc, *off;
    int* bad;
};
hipError_t launch_decode_aggregated(const DecodeArgs& a, hipStream_t st);
// a replay memory's agent rows from its compact records
hipError_t launch_regen_agent_rows(const RegenArgs& g, hipStream_t s);
// offer rows -> their records' templates (from each record's row 0) and slot pairs, and back (every row written whole)
hipError_t launch_offer_compress(const OffRowsArgs& g, hipStream_t s);
hipError_t launch_offer_expand(const OffRowsArgs& g, hipStream_t s);

}  // namespace ms

// ms_action_hist.h — launch arguments and launcher of the action histogram kernel (action_hist_kernels.hip), shared
// with capi.cpp, which checks the arguments and fills the struct; the kernel takes it as it is. No device code here.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ms {

constexpr int kHistMaxActions = 64;      // n_actions the kernel takes
constexpr int kHistMaxCounters = 16383;  // n_bins * n_actions: the workgroup's private counters (and one more word:
                                         // 64 KiB of LDS); cfg4's acceptors take 256 * 49 = 12544

// k_action_hist: counts += the histogram of int8 actions over rows r = t * E + e, t < n_rounds; a row lands in slot
// ((round0 + t) / episode_length) % n_slots of counts [n_slots][n_bins][n_actions]. Element (r, u) of `actions` sits
// at r * row_stride + u * unit_stride, of `select` at r * sel_row_stride + u * sel_unit_stride.
struct ActionHist {
    int mode;               // MS_HIST_ALL / MS_HIST_GATED / MS_HIST_OWNER (marlsched.h)
    int by_unit;            // owner mode: the action of core c's owner o is at unit (o - 1) * C + c (else at c)
    const int8_t* actions;
    int64_t row_stride, unit_stride;
    const int8_t* select;   // gated: the gate [R][U]; owner: core_owner [R][C]; all: unused
    int64_t sel_row_stride, sel_unit_stride;
    int n_cols;             // what a row is scanned over: U (all, gated), C (owner)
    int n_agents, n_cores;  // owner mode (bins N * C)
    int n_bins, n_actions;
    int64_t E;
    int n_rounds, episode_length, n_slots;
    int64_t round0;
    unsigned long long* counts;  // int64 [n_slots][n_bins][n_actions]: added into, never zeroed
    unsigned long long* bad;     // int64, or NULL: += values out of range (they are not binned)
};

// One launch. InvalidValue: a shape the kernel does not take (n_actions, counters, lengths), nothing launched.
hipError_t launch_action_hist(const ActionHist& a, hipStream_t st);

}  // namespace ms

// ms_action_table.h — launch arguments and launcher of the action-by-key table kernel (action_table_kernels.hip),
// shared with capi.cpp, which checks the arguments and fills the struct; the kernel takes it as it is. No device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ms {

constexpr int kTableMaxActions = 64;      // n_actions the kernel takes (the lanes of a wave)
constexpr int kTableMaxKeys = 64;         // n_keys
constexpr int kTableMaxCounters = 16383;  // n_bins * n_keys * n_actions: the workgroup's private counters (the
                                          // histogram's budget, 64 KiB of LDS)

// k_action_table: counts += the joint histogram of (key - key_min, action) over rows r = t * E + e, t < n_rounds; a
// row lands in slot ((round0 + t) / episode_length) % n_slots of counts [n_slots][n_bins][n_keys][n_actions], unit u
// in bin u / units_per_bin. Element (r, u) of `actions` sits at r * row_stride + u * unit_stride, of `keys` at
// r * key_row_stride + u * key_unit_stride (bytes).
struct ActionTable {
    const int8_t* actions;
    int64_t row_stride, unit_stride;
    const int8_t* keys;
    int64_t key_row_stride, key_unit_stride;
    int n_units, units_per_bin, n_bins;
    int n_keys, key_min, n_actions;
    int64_t E;
    int n_rounds, episode_length, n_slots;
    int64_t round0;
    unsigned long long* counts;   // int64 [n_slots][n_bins][n_keys][n_actions]: added into, never zeroed
    unsigned long long* skipped;  // int64, or NULL: += elements whose key is outside [key_min, key_min + n_keys)
    unsigned long long* bad;      // int64, or NULL: += elements with a key in range and an action out of range
};

// One launch. InvalidValue: a shape the kernel does not take (n_actions, n_keys, counters, lengths), nothing launched.
hipError_t launch_action_table(const ActionTable& a, hipStream_t st);

}  // namespace ms

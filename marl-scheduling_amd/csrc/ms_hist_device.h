// ms_hist_device.h — what the two counting kernels share (action_hist_kernels.hip, action_table_kernels.hip): the
// walk's constants, the loads of a row's columns and the count-by-value of a wave. Device code, integers only;
// included by those two units alone.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ms {

namespace {

constexpr int kHistThreads = 256;
constexpr int kHistWords = 8;    // dwords of a row a lane holds at a time: 32 columns
constexpr int kHistBits = 6;     // bits of an action below kHistMaxActions
constexpr int kHistBlocks = 1024;        // workgroups of a launch, about (4 per CU: the LDS holds them)
constexpr int kHistRowsPerBlock = 2048;  // ... of at least this many rows each, so a flush pays for itself

// Columns c0 .. c0 + 3 of a row as the bytes of one word. vec: one aligned dword load (unit stride 1, whole words);
// otherwise a byte load per column inside the row. A lane outside the rows loads nothing.
__device__ __forceinline__ uint32_t load4(const int8_t* __restrict__ p, int64_t row_off, int64_t unit_stride, int c0,
                                          int n_cols, bool vec, bool live) {
    if (!live) return 0;
    if (vec) return *reinterpret_cast<const uint32_t*>(p + row_off + c0);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; j++)
        if (c0 + j < n_cols) w |= (uint32_t)(uint8_t)p[row_off + (int64_t)(c0 + j) * unit_stride] << (8 * j);
    return w;
}

// The wave's 64 values of one column, counted by value: after match(v), lane l's (lo, hi) is the mask of the lanes
// whose v equals l, for values in [0, 2^bits); a lane l >= 2^bits matches nothing. Bit k of v is balloted once; lane
// l keeps the lanes that agree with bit k of l. count(m) is then the number of lanes of the wave-uniform mask m that hold this lane's number.
struct ValueCount {
    uint32_t bit[kHistBits];  // all ones where bit k of the lane number is set
    uint32_t any;             // all ones in the lanes that stand for a value
    uint32_t lo, hi;
    int bits;
    __device__ __forceinline__ ValueCount(int lane, int bits_) : bits(bits_) {
#pragma unroll
        for (int k = 0; k < kHistBits; k++) bit[k] = 0u - ((uint32_t)(lane >> k) & 1u);
        any = lane < (1 << bits) ? 0xffffffffu : 0u;
    }
    __device__ __forceinline__ void match(int v) {
        lo = hi = any;
#pragma unroll
        for (int k = 0; k < kHistBits; k++)
            if (k < bits) {  // (the same for every lane)
                const unsigned long long b = __ballot((v >> k) & 1);
                lo &= ~((uint32_t)b ^ bit[k]);
                hi &= ~((uint32_t)(b >> 32) ^ bit[k]);
            }
    }
    __device__ __forceinline__ uint32_t count(unsigned long long m) const {
        return __popc(lo & (uint32_t)m) + __popc(hi & (uint32_t)(m >> 32));
    }
};

// (host) whether load4 may take whole words of this view
inline bool word_loads(const int8_t* p, int64_t row_stride, int64_t unit_stride, int n_cols) {
    return unit_stride == 1 && n_cols % 4 == 0 && row_stride % 4 == 0 && reinterpret_cast<uintptr_t>(p) % 4 == 0;
}

}  // namespace

}  // namespace ms

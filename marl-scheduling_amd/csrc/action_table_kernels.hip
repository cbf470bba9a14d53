// action_table_kernels.hip — per-episode joint histograms, key x action, of the int8 actions a rollout (or an
// evaluation round) wrote and the int8 key that sits beside each of them in the rings (the job priority of an offer
// slot, byte 2 of the price chooser's state), on gfx950: integer counts only, so the result is exact and the same
// from run to run (ms_action_table in marlsched.h).
//
// The walk is k_action_hist's (action_hist_kernels.hip): a workgroup takes rows of ONE episode (one slot of counts),
// a lane takes a row and the wave walks the row's columns together, the counters are private to the workgroup in the
// LDS and every non-zero one is added to the global counts once. At every step the 64 lanes hold 64 rows' (key,
// action) of one column. The wave counts the actions by value first (ValueCount: lane v learns which rows hold action
// v), then takes the keys that are present one after the other: the first valid lane's key is broadcast, one ballot
// finds the rows that share it, the lanes with a count add it to that key's n_actions consecutive counters, and the
// rows are struck off. That is one ballot and one LDS add per DISTINCT key of the column, every lane on an address of
// its own: 64 rows of one priority under a converged policy cost one add, six priorities cost six, and the n_keys
// that are absent cost nothing (a loop over all keys, as the histogram's over owners, would pay for 64).
// A key is compared before it is used: the broadcast key comes from a lane whose key passed the range check, and a
// lane adds to counter `lane` only where a valid row holds action `lane` < n_actions. An element whose key is out of
// range has its action byte loaded with the row's word but never looked at.
#include <hip/hip_runtime.h>

#include "../../include/marlsched.h"
#include "ms_action_table.h"
#include "ms_hist_device.h"

namespace ms {

namespace {

__global__ void __launch_bounds__(kHistThreads) k_action_table(const ActionTable a, int blocks_per_episode, int vec_a,
                                                               int vec_k) {
    extern __shared__ uint32_t h[];  // [n_bins][n_keys][n_actions] counters
    const int tid = threadIdx.x, lane = tid & 63;
    const int A = a.n_actions, K = a.n_keys, KA = K * A;
    const int n_ctr = a.n_bins * KA;
    for (int i = tid; i < n_ctr; i += kHistThreads) h[i] = 0;
    __syncthreads();
    // the episode of this workgroup and its rounds inside the call
    const int seg = blockIdx.x / blocks_per_episode, x = blockIdx.x - seg * blocks_per_episode;
    const int64_t L = a.episode_length;
    const int64_t k = a.round0 / L + seg;
    int64_t t0 = k * L - a.round0, t1 = (k + 1) * L - a.round0;
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > a.n_rounds ? a.n_rounds : t1;
    const int64_t r1 = t1 * a.E;
    int bits = 1;
    while ((1 << bits) < A) bits++;
    ValueCount vc(lane, bits);
    uint32_t n_skip = 0, n_bad = 0;  // of the wave (the same in every lane)
    for (int64_t base = t0 * a.E + (int64_t)x * kHistThreads; base < r1;
         base += (int64_t)blocks_per_episode * kHistThreads) {
        const int64_t r = base + tid;
        const bool in = r < r1;
        const int64_t ao = r * a.row_stride, ko = r * a.key_row_stride;
        int bin = 0, in_bin = 0;  // of the column: bin = c / units_per_bin, kept by counting (c only ever steps by one)
        for (int c0 = 0; c0 < a.n_units; c0 += 4 * kHistWords) {
            uint32_t wa[kHistWords], wk[kHistWords];
#pragma unroll
            for (int i = 0; i < kHistWords; i++) {
                const int c = c0 + 4 * i;
                const bool live = in && c < a.n_units;
                wa[i] = load4(a.actions, ao, a.unit_stride, c, a.n_units, vec_a, live);
                wk[i] = load4(a.keys, ko, a.key_unit_stride, c, a.n_units, vec_k, live);
            }
#pragma unroll
            for (int i = 0; i < kHistWords; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int c = c0 + 4 * i + j;
                    if (c < a.n_units) {  // (the same for every lane)
                        const int key = (int)(int8_t)(wk[i] >> (8 * j)) - a.key_min;
                        const bool keyed = in && (unsigned)key < (unsigned)K;
                        const int act = keyed ? (int)(int8_t)(wa[i] >> (8 * j)) : 0;
                        const bool valid = keyed && (unsigned)act < (unsigned)A;
                        n_skip += __popcll(__ballot(in && !keyed));
                        n_bad += __popcll(__ballot(keyed && !valid));
                        unsigned long long rem = __ballot(valid);
                        if (rem) {  // (the same for every lane)
                            // lane l < A: which of the wave's rows took action l in this column
                            vc.match(act);
                            uint32_t* hc = h + bin * KA;
                            do {  // the keys present among the valid rows, one ballot each
                                const int kk = __builtin_amdgcn_readlane(key, __ffsll(rem) - 1);
                                const unsigned long long m = __ballot(valid && key == kk);
                                const uint32_t n = vc.count(m);
                                if (n) atomicAdd(&hc[kk * A + lane], n);
                                rem &= ~m;
                            } while (rem);
                        }
                        if (++in_bin == a.units_per_bin) in_bin = 0, bin++;
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned long long* out = a.counts + (uint64_t)(k % a.n_slots) * (uint64_t)n_ctr;
    for (int i = tid; i < n_ctr; i += kHistThreads) {
        const uint32_t v = h[i];
        if (v) atomicAdd(&out[i], (unsigned long long)v);
    }
    if (lane == 0) {  // (a wave's two counts, once)
        if (n_skip && a.skipped) atomicAdd(a.skipped, (unsigned long long)n_skip);
        if (n_bad && a.bad) atomicAdd(a.bad, (unsigned long long)n_bad);
    }
}

}  // namespace

hipError_t launch_action_table(const ActionTable& a, hipStream_t st) {
    if (a.n_actions < 1 || a.n_actions > kTableMaxActions || a.n_keys < 1 || a.n_keys > kTableMaxKeys)
        return hipErrorInvalidValue;
    if (a.key_min < -128 || a.key_min > 127) return hipErrorInvalidValue;
    if (a.n_units < 1 || a.units_per_bin < 1 || a.n_units % a.units_per_bin != 0 ||
        a.n_bins != a.n_units / a.units_per_bin)
        return hipErrorInvalidValue;
    if ((int64_t)a.n_bins * a.n_keys * a.n_actions > kTableMaxCounters) return hipErrorInvalidValue;
    if (a.E < 1 || a.n_rounds < 1 || a.episode_length < 1 || a.n_slots < 1 || a.round0 < 0) return hipErrorInvalidValue;
    if (a.row_stride < 1 || a.unit_stride < 1 || a.key_row_stride < 1 || a.key_unit_stride < 1) return hipErrorInvalidValue;
    if (!a.actions || !a.keys || !a.counts) return hipErrorInvalidValue;
    const int64_t L = a.episode_length, T = a.n_rounds;
    const int64_t n_episodes = (a.round0 + T - 1) / L - a.round0 / L + 1;
    const int64_t rows = (T < L ? T : L) * a.E;  // of the call's longest episode
    int64_t per = (rows + kHistRowsPerBlock - 1) / kHistRowsPerBlock;
    const int64_t cap = n_episodes >= kHistBlocks ? 1 : kHistBlocks / n_episodes;
    per = per > cap ? cap : per;
    // a workgroup's private counters are 32 bits wide: its share of the rows times the columns stays below 2^32
    if (n_episodes * per > 0x7fffffffll || (rows + per - 1) / per >= (1ll << 32) / a.n_units) return hipErrorInvalidValue;
    const int vec_a = word_loads(a.actions, a.row_stride, a.unit_stride, a.n_units);
    const int vec_k = word_loads(a.keys, a.key_row_stride, a.key_unit_stride, a.n_units);
    const size_t lds = (size_t)a.n_bins * a.n_keys * a.n_actions * sizeof(uint32_t);
    hipLaunchKernelGGL(k_action_table, dim3((unsigned)(n_episodes * per)), dim3(kHistThreads), lds, st, a, (int)per,
                       vec_a, vec_k);
    return hipGetLastError();
}

}  // namespace ms

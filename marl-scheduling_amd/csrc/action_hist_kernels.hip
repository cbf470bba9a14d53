// action_hist_kernels.hip — per-episode histograms of the int8 actions a rollout (or an evaluation round) wrote, on
// gfx950: integer counts only, so the result is exact and the same from run to run. One kernel, three ways to
// select what is counted (ms_action_hist in marlsched.h): every element, the elements a gate byte marks, or the
// acceptor action of each core's owner.
//
// A workgroup takes rows of ONE episode (one slot of counts), counts them into private LDS counters and adds every
// non-zero counter to the global counts once. A lane takes a row and the wave walks the row's columns together, so
// at every step the 64 lanes hold 64 rows' values of one column: under a converged or greedy policy all the same
// counter. The wave therefore counts by value before it touches the LDS (ValueCount): lane v learns how many of the
// 64 rows hold action v, from one ballot per bit of the value, and the lanes with a count add it to the column's
// n_actions consecutive counters: one LDS add per column and wave, every lane on an address of its own, whatever
// the policy. (n_actions <= 64, the lanes of a wave, is where the limit comes from.)
#include <hip/hip_runtime.h>

#include "../../include/marlsched.h"
#include "ms_action_hist.h"
#include "ms_hist_device.h"

namespace ms {

namespace {

template <int MODE>
__global__ void __launch_bounds__(kHistThreads) k_action_hist(const ActionHist a, int blocks_per_episode, int vec_a,
                                                              int vec_s) {
    extern __shared__ uint32_t h[];  // [n_bins * n_actions] counters, then the out-of-range count
    const int tid = threadIdx.x, lane = tid & 63;
    const int n_ctr = a.n_bins * a.n_actions;
    for (int i = tid; i <= n_ctr; i += kHistThreads) h[i] = 0;
    __syncthreads();
    // the episode of this workgroup and its rounds inside the call
    const int seg = blockIdx.x / blocks_per_episode, x = blockIdx.x - seg * blocks_per_episode;
    const int64_t L = a.episode_length;
    const int64_t k = a.round0 / L + seg;
    int64_t t0 = k * L - a.round0, t1 = (k + 1) * L - a.round0;
    t0 = t0 < 0 ? 0 : t0;
    t1 = t1 > a.n_rounds ? a.n_rounds : t1;
    const int64_t r1 = t1 * a.E;
    const int A = a.n_actions, N = a.n_agents, C = a.n_cores;
    int bits = 1;
    while ((1 << bits) < A) bits++;
    ValueCount vc(lane, bits);
    for (int64_t base = t0 * a.E + (int64_t)x * kHistThreads; base < r1;
         base += (int64_t)blocks_per_episode * kHistThreads) {
        const int64_t r = base + tid;
        const bool in = r < r1;
        const int64_t ao = r * a.row_stride, so = r * a.sel_row_stride;
        for (int c0 = 0; c0 < a.n_cols; c0 += 4 * kHistWords) {
            uint32_t wa[kHistWords], ws[kHistWords];
#pragma unroll
            for (int i = 0; i < kHistWords; i++) {
                const int c = c0 + 4 * i;
                const bool live = in && c < a.n_cols;
                wa[i] = ws[i] = 0;
                if (MODE != MS_HIST_OWNER || !a.by_unit)
                    wa[i] = load4(a.actions, ao, a.unit_stride, c, a.n_cols, vec_a, live);
                if (MODE != MS_HIST_ALL) ws[i] = load4(a.select, so, a.sel_unit_stride, c, a.n_cols, vec_s, live);
            }
#pragma unroll
            for (int i = 0; i < kHistWords; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int c = c0 + 4 * i + j;
                    if (c < a.n_cols) {  // (the same for every lane)
                        bool valid = in, bad = false;
                        int act = (int)(int8_t)(wa[i] >> (8 * j));
                        const int sel = (int)(int8_t)(ws[i] >> (8 * j));
                        if (MODE == MS_HIST_GATED) valid = in && sel != 0;
                        if (MODE == MS_HIST_OWNER) {
                            // owner 0 is the auctioneer: skipped; an owner outside [0, N] forms no index
                            valid = in && sel > 0 && sel <= N;
                            bad = in && (sel < 0 || sel > N);
                            if (a.by_unit)
                                act = valid ? (int)a.actions[ao + (int64_t)((sel - 1) * C + c) * a.unit_stride] : 0;
                        }
                        if (valid && (unsigned)act >= (unsigned)A) valid = false, bad = true;
                        // lane l < A: how many of the wave's valid rows took action l in this column
                        vc.match(act);
                        if (MODE == MS_HIST_OWNER) {
                            for (int o = 1; o <= N; o++) {  // the rows of one owner share a bin
                                const unsigned long long m = __ballot(valid && sel == o);
                                if (m) {
                                    const uint32_t n = vc.count(m);
                                    if (n) atomicAdd(&h[((o - 1) * C + c) * A + lane], n);
                                }
                            }
                        } else {
                            const uint32_t n = vc.count(__ballot(valid));
                            if (n) atomicAdd(&h[c * A + lane], n);
                        }
                        if (__ballot(bad) && bad) atomicAdd(&h[n_ctr], 1u);  // (one add of the lane count per wave)
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
    if (tid == 0 && h[n_ctr] && a.bad) atomicAdd(a.bad, (unsigned long long)h[n_ctr]);
}

}  // namespace

hipError_t launch_action_hist(const ActionHist& a, hipStream_t st) {
    if (a.mode != MS_HIST_ALL && a.mode != MS_HIST_GATED && a.mode != MS_HIST_OWNER) return hipErrorInvalidValue;
    if (a.n_actions < 1 || a.n_actions > kHistMaxActions || a.n_bins < 1 || a.n_cols < 1) return hipErrorInvalidValue;
    if ((int64_t)a.n_bins * a.n_actions > kHistMaxCounters) return hipErrorInvalidValue;
    if (a.E < 1 || a.n_rounds < 1 || a.episode_length < 1 || a.n_slots < 1 || a.round0 < 0) return hipErrorInvalidValue;
    if (a.mode == MS_HIST_OWNER && (a.n_agents < 1 || a.n_agents > 127 || a.n_cores != a.n_cols ||
                                    a.n_bins != a.n_agents * a.n_cores))
        return hipErrorInvalidValue;
    if (a.mode != MS_HIST_OWNER && a.n_bins != a.n_cols) return hipErrorInvalidValue;
    if (!a.actions || !a.counts || (a.mode != MS_HIST_ALL && !a.select)) return hipErrorInvalidValue;
    const int64_t L = a.episode_length, T = a.n_rounds;
    const int64_t n_episodes = (a.round0 + T - 1) / L - a.round0 / L + 1;
    const int64_t rows = (T < L ? T : L) * a.E;  // of the call's longest episode
    int64_t per = (rows + kHistRowsPerBlock - 1) / kHistRowsPerBlock;
    const int64_t cap = n_episodes >= kHistBlocks ? 1 : kHistBlocks / n_episodes;
    per = per > cap ? cap : per;
    // a workgroup's private counters are 32 bits wide: its share of the rows times the columns stays below 2^32
    if (n_episodes * per > 0x7fffffffll || (rows + per - 1) / per >= (1ll << 32) / a.n_cols) return hipErrorInvalidValue;
    const int vec_a = !(a.mode == MS_HIST_OWNER && a.by_unit) && word_loads(a.actions, a.row_stride, a.unit_stride, a.n_cols);
    const int vec_s = a.mode != MS_HIST_ALL && word_loads(a.select, a.sel_row_stride, a.sel_unit_stride, a.n_cols);
    auto kern = a.mode == MS_HIST_ALL ? k_action_hist<MS_HIST_ALL>
                                      : a.mode == MS_HIST_GATED ? k_action_hist<MS_HIST_GATED> : k_action_hist<MS_HIST_OWNER>;
    const size_t lds = ((size_t)a.n_bins * a.n_actions + 1) * sizeof(uint32_t);
    hipLaunchKernelGGL(kern, dim3((unsigned)(n_episodes * per)), dim3(kHistThreads), lds, st, a, (int)per, vec_a, vec_s);
    return hipGetLastError();
}

}  // namespace ms

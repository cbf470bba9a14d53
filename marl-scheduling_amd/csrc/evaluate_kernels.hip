// evaluate_kernels.hip — ActorCritic.evaluate(state, action) for gfx950 (PPOmodules.py:65-72): the
// log-probability of a given action, the state value and the entropy of the policy, per observation row.
//
// k_evaluate: ActorCritic.actor's forward on the primitives of ms_act.h, exactly as k_act runs it
// (policy_kernels.hip: 16 observation rows per MFMA tile, the exact three-term bf16 layer 1, layers 2-3 on
// v_mfma_f32_16x16x4_f32), then the softmax as Head::run2 takes it (exp2 of the logit minus the row's maximum,
// the lane sums added across the row's four lanes, one reciprocal) and, in place of the inverse CDF,
//   logprob = log(clamp(p[a], eps, 1 - eps))               (Head::clamped_log: what k_act writes for its sample)
//   entropy = -sum_k log(clamp(p[k], eps, 1 - eps)) p[k]   (Categorical.entropy on clamped logits)
// The critic (Linear-tanh-Linear-tanh-Linear of width 1) runs as a second head, a Head<1> with its own layer-1
// terms, on the row the wave already holds. No random number is read; act_frag and row_base are ignored.
//
// A row's probabilities sit in 4 lanes x 4 registers per 16-action tile: lane (j, g4) of the wave holds
// actions 16 t + 4 g4 + q of row j. Padding actions (A is rarely a multiple of 16) read a -inf logit
// (Head::load's bias), so their numerator is 0 and drops out of the sum; the entropy skips them by index.
// The action byte is only compared with the lane's action indices, never used as an address: a byte outside
// [0, A) reads nothing and the row's logprob is NaN (value and entropy do not depend on it).
//
// Which outputs are wanted is a wave-uniform run-time branch of one kernel per shape bucket, so an output is
// computed by the same instructions whichever others are requested, and a head nobody asks for is neither
// loaded nor run.
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/marlsched.h"
#include "ms_act_kernels.h"  // load_row, W1Split, Head, s1_bucket, nt_bucket, tile_blocks
#include "ms_evaluate.h"

// the shared headers contract freely (their code rounds as k_act's); this unit's own arithmetic fuses only
// where an expression says fmaf (build.sh: -ffp-contract=on for this file)
#pragma clang fp contract(on)

namespace ms {

// One wave = a contiguous range of 16-row tiles of one group (the next tile's rows and actions prefetched in
// registers); no LDS.
template <int S1, int NT>
__global__ void __launch_bounds__(256) k_evaluate(EvalArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int gw = (int)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = gw / a.waves_per_group;
    const int wv = gw - grp * a.waves_per_group;
    if (grp >= a.actor.n_groups) return;
    const int j = lane & 15, g4 = lane >> 4;
    const bool want_lp = a.logprob != nullptr, want_ent = a.entropy != nullptr, want_v = a.value != nullptr;
    const bool want_actor = want_lp || want_ent;  // (all wave-uniform)
    // 32-bit byte offsets into bounds-checked buffers (sizes checked at the launch)
    const long long n_rows = (long long)a.E * a.U;
    const RawBuf obs_b(a.obs, n_rows * a.stride), act_b(a.actions, want_lp ? n_rows : 0);
    const RawBuf lp_b(a.logprob, want_lp ? 4 * n_rows : 0), v_b(a.value, want_v ? 4 * n_rows : 0),
        ent_b(a.entropy, want_ent ? 4 * n_rows : 0);
    W1Split<S1> w1, w1c;
    Head<NT> h1;
    Head<1> hc;
    if (want_actor) {
        w1.load(a.actor.w1 + (size_t)grp * 16 * a.actor.in_dim, a.actor.in_dim, j, g4);
        h1.load(a.actor, grp, j, g4);
    }
    if (want_v) {
        w1c.load(a.critic.w1 + (size_t)grp * 16 * a.critic.in_dim, a.critic.in_dim, j, g4);
        hc.load(a.critic, grp, j, g4);  // (n_actions = 1: accumulator row 0 is the value)
    }
    const int A = a.actor.n_actions;
    const int stride4 = a.stride >> 2;
    const int tiles = (a.n_items + 15) >> 4;
    const int t0 = wv * a.tiles_per_wave;
    const int t1 = min(t0 + a.tiles_per_wave, tiles);
    // item i of this group -> obs row (-1 past the end)
    auto row_of = [&](int tile) -> int {
        const int i = tile * 16 + j;
        if (i >= a.n_items) return -1;
        const int e = i / a.S;
        return e * a.U + grp * a.S + (i - e * a.S);
    };
    uint32_t pre[S1][2];
    int row = -1, pre_act = 0;
    auto fetch = [&](int tile) {
        row = row_of(tile);
        const uint32_t r = (uint32_t)(row < 0 ? 0 : row);
        load_row<S1>(obs_b, r * (uint32_t)a.stride, stride4, g4, pre);
        if (want_lp) pre_act = act_b.ld8s(r);
    };
    if (t0 < t1) fetch(t0);
    for (int tile = t0; tile < t1; tile++) {
        uint32_t xd[S1][2];
#pragma unroll
        for (int s = 0; s < S1; s++) xd[s][0] = pre[s][0], xd[s][1] = pre[s][1];
        const int cur = row, act = pre_act;
        if (tile + 1 < t1) fetch(tile + 1);
        const bool store = cur >= 0 && g4 == 0;
        if (want_actor) {
            float z[NT][4];
            const float m = rows_max(h1.logits(w1.layer1(xd), z));
            // the numerators and their sum as Head::run2 forms them (lane sums per tile, then over tiles,
            // then the row's four lanes)
            const float m_l2e = m * 1.4426950408889634f;
            float S = 0.f, bs[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                bs[t] = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    z[t][q] = fast_exp_sub(z[t][q], m_l2e);
                    bs[t] += z[t][q];
                }
            }
#pragma unroll
            for (int t = 0; t < NT; t++) S += bs[t];
            S = rows_sum(S);
            const float rS = __builtin_amdgcn_rcpf(S);
            if (want_lp) {
                float mine = 0.f;
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int q = 0; q < 4; q++) mine = (16 * t + 4 * g4 + q == act) ? z[t][q] : mine;
                mine = rows_sum(mine);
                float lp = Head<NT>::clamped_log(mine * rS);
                if (act < 0 || act >= A) lp = __builtin_nanf("");  // no such action
                if (store) lp_b.stf(4u * (uint32_t)cur, lp);
            }
            if (want_ent) {
                float ent = 0.f;
#pragma unroll
                for (int t = 0; t < NT; t++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const float p = z[t][q] * rS;
                        const float term = fmaf(Head<NT>::clamped_log(p), p, ent);
                        ent = 16 * t + 4 * g4 + q < A ? term : ent;  // padding: nothing
                    }
                ent = rows_sum(ent);
                if (store) ent_b.stf(4u * (uint32_t)cur, -ent);
            }
        }
        if (want_v) {
            float zc[1][4];
            hc.logits(w1c.layer1(xd), zc);
            if (store) v_b.stf(4u * (uint32_t)cur, zc[0][0]);  // lane (j, 0), register 0: output 0 of row j
        }
    }
}

constexpr long long kEvalWaves = 4096;

// every array is addressed with 31-bit byte offsets (RawBuf), rows and items with ints
static bool evaluate_fits(const EvalArgs& a) {
    const long long rows = (long long)a.E * a.U;
    const ms_mlp_params& p = a.actor;
    return a.E >= 1 && rows <= 0x7fffffffll && rows * a.stride <= 0x7fffffffll && rows * 4 <= 0x7fffffffll &&
           a.stride >= 4 && (a.stride & 3) == 0 && a.stride <= 256 && p.in_dim >= 1 && p.in_dim <= a.stride &&
           p.hidden == 16 && p.n_actions >= 1 && p.n_actions <= 127 && a.S >= 1 && p.n_groups >= 1 &&
           (long long)a.S * p.n_groups == a.U && a.n_items == a.E * a.S;
}

template <int S1>
static hipError_t launch_evaluate_s(EvalArgs& a, hipStream_t st) {
    const unsigned blocks = tile_blocks(a.n_items, a.actor.n_groups, kEvalWaves, &a.tiles_per_wave, &a.waves_per_group);
    switch (nt_bucket(a.actor.n_actions)) {
        case 1: hipLaunchKernelGGL((k_evaluate<S1, 1>), dim3(blocks), dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_evaluate<S1, 2>), dim3(blocks), dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_evaluate<S1, 4>), dim3(blocks), dim3(256), 0, st, a); break;
        case 8: hipLaunchKernelGGL((k_evaluate<S1, 8>), dim3(blocks), dim3(256), 0, st, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t dispatch_evaluate(EvalArgs& a, hipStream_t st) {
    if (!evaluate_fits(a) || !a.obs) return hipErrorInvalidValue;
    if (a.logprob && !a.actions) return hipErrorInvalidValue;
    if (a.value && (a.critic.hidden != 16 || a.critic.n_actions != 1 || a.critic.in_dim != a.actor.in_dim ||
                    a.critic.n_groups != a.actor.n_groups))
        return hipErrorInvalidValue;
    if (!a.logprob && !a.value && !a.entropy) return hipSuccess;  // nothing asked for
    switch (s1_bucket(a.stride)) {
        case 1: return launch_evaluate_s<1>(a, st);
        case 2: return launch_evaluate_s<2>(a, st);
        case 4: return launch_evaluate_s<4>(a, st);
        case 8: return launch_evaluate_s<8>(a, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace ms

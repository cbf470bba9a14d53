// greedy_kernels.hip — deterministic (argmax) action selection for gfx950: policy evaluation.
//
// k_greedy: ActorCritic.actor's forward (PPOmodules.py:53-63, Linear-tanh-Linear-tanh-Linear) on the
// primitives of ms_act.h, exactly as k_act runs it (policy_kernels.hip: 16 observation rows per MFMA tile,
// the exact three-term bf16 layer 1, layers 2-3 on v_mfma_f32_16x16x4_f32), and then the first maximum of
// the logits (torch.argmax's rule, as dqn_kernels.hip documents for the Q-values) in place of softmax +
// inverse CDF + Philox: no random number is read or advanced, and no exponential is taken unless the
// caller asks for the chosen action's log-prob (logit - logsumexp).
//
// A row's logits sit in 4 lanes x 4 registers per 16-action tile: lane (j, g4) of the wave holds actions
// 16 t + 4 g4 + q of row j. The reduction carries (value, index) through registers, then the row's four
// lanes, and takes the smaller index on equal values at every step, so the first maximum wins within and
// across tiles. Padding actions (A is rarely a multiple of 16) are masked to -inf before the reduction.
//
// k_greedy_common: rows equal to a common row (the acceptor row of a core the agent does not own,
// Agent.py:167-212), given as full rows or in the env's compact form (core rows + owners), take the
// group's common-row action, computed once per wave; the other rows are listed in LDS and run through the
// tiles. The results equal k_greedy's on the full rows bit for bit (an MFMA column does not depend on its
// neighbours, and both kernels run the same code on it).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/marlsched.h"
#include "ms_act_kernels.h"  // the launch-shape helpers shared with the sampling kernels; GreedyArgs: ms_act_args.h

#pragma clang fp contract(fast)  // (build.sh: -ffp-contract=fast for this file)

namespace ms {

constexpr int kGreedySeg = 512;  // most items per wave of k_greedy_common = capacity of its LDS row list

// the logits of the tile's 16 rows from their layer-1 pre-activations (Head::logits), the padding
// actions a = 16 t + 4 g4 + q >= A masked to -inf whatever their bias reads
template <int NT>
__device__ __forceinline__ void greedy_logits(const Head<NT>& h, f4 a1, int A, int g4, float (&z)[NT][4]) {
    h.logits(a1, z, [&](int t, int q, float v) { return 16 * t + 4 * g4 + q < A ? v : -INFINITY; });
}

// The first maximum of row j's logits, on every lane of the row, and (want_lp) its log-prob
// logit - logsumexp = -log(sum exp(z - max)).
template <int NT>
__device__ __forceinline__ void greedy_pick(const float (&z)[NT][4], int g4, bool want_lp, int& action,
                                            float& logprob) {
    // this lane's actions in increasing order: a later one wins only when strictly larger
    float bv = z[0][0];
    int bi = 4 * g4;
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (t == 0 && q == 0) continue;
            if (z[t][q] > bv) {
                bv = z[t][q];
                bi = 16 * t + 4 * g4 + q;
            }
        }
    // the row's four lanes: the larger value, the smaller index between equal values
    uint32_t vv[4], ii[4];
    rows_bcast(__float_as_uint(bv), vv);
    rows_bcast((uint32_t)bi, ii);
    float m = __uint_as_float(vv[0]);
    int mi = (int)ii[0];
#pragma unroll
    for (int k = 1; k < 4; k++) {
        const float v = __uint_as_float(vv[k]);
        const int i = (int)ii[k];
        if (v > m || (v == m && i < mi)) {
            m = v;
            mi = i;
        }
    }
    action = mi;
    logprob = 0.f;
    if (want_lp) {  // wave-uniform
        const float m_l2e = m * 1.4426950408889634f;
        float s = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) s += fast_exp_sub(z[t][q], m_l2e);
        logprob = -fast_log(rows_sum(s));
    }
}

// One wave = a contiguous range of 16-row tiles of one group (the next tile's rows prefetched in registers).
// With a price net (NT2 > 0) the wave is FreePriceOfferPPO.selectAction with both picks greedy.
template <int S1, int NT, int NT2>
__device__ __forceinline__ void greedy_tiles(const GreedyArgs& a, int block) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int gw = block * 4 + __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = gw / a.waves_per_group;
    const int wv = gw - grp * a.waves_per_group;
    if (grp >= a.n1.n_groups) return;
    const int j = lane & 15, g4 = lane >> 4;
    constexpr int NP = NT2 > 0 ? NT2 : 1;
    // 32-bit byte offsets into bounds-checked buffers (sizes checked at the launch)
    const long long n_rows = (long long)a.E * a.U;
    const RawBuf obs_b(a.obs, n_rows * a.stride), act_b(a.action, n_rows), lp_b(a.logprob, a.logprob ? 4 * n_rows : 0);
    const RawBuf pst_b(a.price_state, NT2 > 0 ? 4 * n_rows : 0), pact_b(a.price_action, NT2 > 0 ? n_rows : 0),
        envp_b(a.env_price, NT2 > 0 ? n_rows : 0);
    W1Split<S1> w1;
    Head<NT> h1;
    w1.load(a.n1.w1 + (size_t)grp * 16 * a.n1.in_dim, a.n1.in_dim, j, g4);
    h1.load(a.n1, grp, j, g4);
    // the price chooser as the same kernel would run it on rows of 4 bytes (S1 = 1), so its pick equals
    // ms_policy_act_greedy's on the price_state written here, bit for bit
    Head<NP> h2;
    W1Split<1> w1p;
    if constexpr (NT2 > 0) {
        h2.load(a.n2, grp, j, g4);
        w1p.load(a.n2.w1 + (size_t)grp * 16 * 4, 4, j, g4);
    }
    const bool want_lp = a.logprob != nullptr;
    const int A1 = a.n1.n_actions;
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
    int row = -1;
    if (t0 < t1) {
        row = row_of(t0);
        load_row<S1>(obs_b, (uint32_t)(row < 0 ? 0 : row) * (uint32_t)a.stride, stride4, g4, pre);
    }
    for (int tile = t0; tile < t1; tile++) {
        uint32_t xd[S1][2];
#pragma unroll
        for (int s = 0; s < S1; s++) xd[s][0] = pre[s][0], xd[s][1] = pre[s][1];
        const int cur = row;
        if (tile + 1 < t1) {
            row = row_of(tile + 1);
            load_row<S1>(obs_b, (uint32_t)(row < 0 ? 0 : row) * (uint32_t)a.stride, stride4, g4, pre);
        }
        float z[NT][4];
        greedy_logits<NT>(h1, w1.layer1(xd), A1, g4, z);
        int act;
        float lp;
        greedy_pick<NT>(z, g4, want_lp, act, lp);
        if (cur >= 0 && g4 == 0) {
            act_b.st8((uint32_t)cur, act);
            if (want_lp) lp_b.stf(4u * (uint32_t)cur, lp);
        }
        if constexpr (NT2 > 0) {
            // price chooser input (PPOmodules.py:316-327): lane g4 takes byte g4 of
            // [obs[2a], obs[2a+1], obs[2C], obs[2C+1]], or -5 for a = 0 (a <= C, so the byte lies in the row)
            const int k = g4 < 2 ? 2 * act + g4 : 2 * a.n_cores + (g4 - 2);
            const int byte = obs_b.ld8s((uint32_t)(cur < 0 ? 0 : cur) * (uint32_t)a.stride + (uint32_t)k);
            const int pin = act == 0 ? -5 : byte;
            // the row's 4 bytes as the one dword a 4-byte row is (the clamped loads of load_row repeat it)
            uint32_t pb[4];
            rows_bcast((uint32_t)pin & 0xffu, pb);
            const uint32_t pd = pb[0] | (pb[1] << 8) | (pb[2] << 16) | (pb[3] << 24);
            float z2[NP][4];
            const uint32_t px[1][2] = {{pd, pd}};
            greedy_logits<NP>(h2, w1p.layer1(px), a.n2.n_actions, g4, z2);
            int pact;
            float plp;
            greedy_pick<NP>(z2, g4, false, pact, plp);
            if (cur >= 0) {
                pst_b.st8(4u * (uint32_t)cur + (uint32_t)g4, pin);
                if (g4 == 0) {
                    pact_b.st8((uint32_t)cur, pact);
                    envp_b.st8((uint32_t)cur, act == 0 ? -5 : pact);
                }
            }
        }
    }
}

// One wave = a contiguous range of at most kGreedySeg items of one group. The common row's action is one
// forward per wave; the scan writes it to every item equal to the common row (OWN: every item whose agent
// does not own the core) and lists the others, which then run through the tiles.
template <int S1, int NT, bool OWN>
__device__ __forceinline__ void greedy_common_rows(const GreedyArgs& a, int block) {
    __shared__ int32_t s_list[4][kGreedySeg];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gw = block * 4 + wid;
    const int grp = gw / a.waves_per_group;
    const int wv = gw - grp * a.waves_per_group;
    if (grp >= a.n1.n_groups) return;  // whole waves only: the kernel has no block barrier
    const int j = lane & 15, g4 = lane >> 4;
    const int A = a.n1.n_actions;
    const int stride4 = a.stride >> 2;
    const long long n_rows = (long long)a.E * a.U;
    const long long n_src = OWN ? (long long)a.E * a.n_cores : n_rows;  // observation rows in memory
    const RawBuf obs_b(a.obs, n_src * a.stride), com_b(a.common, a.stride), own_b(a.owner, OWN ? n_src : 0);
    const RawBuf act_b(a.action, n_rows), lp_b(a.logprob, a.logprob ? 4 * n_rows : 0);
    const bool want_lp = a.logprob != nullptr;
    W1Split<S1> w1;
    Head<NT> h1;
    w1.load(a.n1.w1 + (size_t)grp * 16 * a.n1.in_dim, a.n1.in_dim, j, g4);
    h1.load(a.n1, grp, j, g4);
    // the common row's action (every column of the tile is the common row)
    int c_act;
    float c_lp;
    {
        uint32_t xd[S1][2];
        load_row<S1>(com_b, 0u, stride4, g4, xd);
        float z[NT][4];
        greedy_logits<NT>(h1, w1.layer1(xd), A, g4, z);
        greedy_pick<NT>(z, g4, want_lp, c_act, c_lp);
    }
    int32_t* list = s_list[wid];
    const int i_begin = wv * a.items_per_wave;
    const int i_end = min(i_begin + a.items_per_wave, a.n_items);  // <= kGreedySeg items
    const uint64_t below = (1ull << lane) - 1ull;
    // the observation row in memory of output row r: r itself, or the core row of (e, u = a*C + c)
    auto src_of = [&](int r, int& agent) -> int {
        if (!OWN) return r;
        const int e = r / a.U, u = r - e * a.U;
        agent = u / a.n_cores;
        return e * a.n_cores + (u - agent * a.n_cores);
    };
    int n_list = 0;
    for (int i0 = i_begin; i0 < i_end; i0 += 64) {
        const int i = i0 + lane;
        const bool in = i < i_end;
        const int e = (in ? i : 0) / a.S;
        const int row = in ? e * a.U + grp * a.S + (i - e * a.S) : 0;
        int agent = 0;
        const int src = src_of(row, agent);
        bool common;
        if constexpr (OWN) {
            common = own_b.ld8s((uint32_t)src) != agent + 1;
        } else {
            common = true;
            const uint32_t rb = (uint32_t)src * (uint32_t)a.stride;
            for (int d = 0; d < stride4; d++) common = common && obs_b.ld32(rb + 4u * d) == com_b.ld32(4u * d);
        }
        if (in && common) {
            act_b.st8((uint32_t)row, c_act);
            if (want_lp) lp_b.stf(4u * (uint32_t)row, c_lp);
        }
        const bool other = in && !common;
        const uint64_t m = __ballot(other);
        if (other) list[n_list + __popcll(m & below)] = row;
        n_list += __popcll(m);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int t0 = 0; t0 < n_list; t0 += 16) {
        const bool valid = t0 + j < n_list;
        const int row = list[valid ? t0 + j : t0];  // (a tail column repeats the tile's first row; not stored)
        int agent = 0;
        const int src = src_of(row, agent);
        uint32_t xd[S1][2];
        load_row<S1>(obs_b, (uint32_t)src * (uint32_t)a.stride, stride4, g4, xd);
        float z[NT][4];
        greedy_logits<NT>(h1, w1.layer1(xd), A, g4, z);
        int act;
        float lp;
        greedy_pick<NT>(z, g4, want_lp, act, lp);
        if (valid && g4 == 0) {
            act_b.st8((uint32_t)row, act);
            if (want_lp) lp_b.stf(4u * (uint32_t)row, lp);
        }
    }
}

template <int S1, int NT, int NT2>
__global__ void __launch_bounds__(256) k_greedy(GreedyArgs a) {
    greedy_tiles<S1, NT, NT2>(a, blockIdx.x);
}

template <int S1, int NT, bool OWN>
__global__ void __launch_bounds__(256) k_greedy_common(GreedyArgs a) {
    greedy_common_rows<S1, NT, OWN>(a, blockIdx.x);
}

// a round's offer units (the first off_blocks blocks) and compact acceptors in one launch, as k_act_pair
template <int S1a, int NTa, int NT2a, int S1b, int NTb>
__global__ void __launch_bounds__(256) k_greedy_pair(GreedyArgs off, GreedyArgs acc, int off_blocks) {
    if ((int)blockIdx.x < off_blocks)
        greedy_tiles<S1a, NTa, NT2a>(off, blockIdx.x);
    else
        greedy_common_rows<S1b, NTb, true>(acc, (int)blockIdx.x - off_blocks);
}

// ---- launch shapes (tile_blocks, common_blocks: ms_act_kernels.h); the scan has no draws to pair up, so
//      a wave takes whole single 64-item steps
static unsigned greedy_tile_blocks(GreedyArgs& a, long long target) {
    return tile_blocks(a.n_items, a.n1.n_groups, target, &a.tiles_per_wave, &a.waves_per_group);
}
static unsigned greedy_common_blocks(GreedyArgs& a, long long target) {
    return common_blocks(a.n_items, a.n1.n_groups, target, 64, kGreedySeg, &a.items_per_wave, &a.waves_per_group);
}

constexpr long long kGreedyWaves = 4096, kGreedyCommonWaves = 2048;

// every array is addressed with 31-bit byte offsets (RawBuf), rows and items with ints
static bool greedy_fits(const GreedyArgs& a) {
    const long long rows = (long long)a.E * a.U;
    return rows * a.stride <= 0x7fffffffll && rows * 4 <= 0x7fffffffll && a.stride >= 4 && (a.stride & 3) == 0 &&
           a.stride <= 256 && a.n1.in_dim <= a.stride && a.n1.hidden == 16 && a.n1.n_actions >= 1 &&
           a.n1.n_actions <= 128 && a.S >= 1 && a.n1.n_groups >= 1 && (long long)a.S * a.n1.n_groups == a.U;
}

template <int S1, int NT>
static hipError_t launch_greedy_t(GreedyArgs& a, hipStream_t st) {
    if (a.n2.n_groups > 0) {
        // the core chooser has C + 1 <= 64 actions wherever the price chooser's input fits the row
        if constexpr (NT <= 4) {
            const int nt2 = nt_bucket(a.n2.n_actions);
            const unsigned blocks = greedy_tile_blocks(a, kGreedyWaves);
            if (nt2 == 1)
                hipLaunchKernelGGL((k_greedy<S1, NT, 1>), dim3(blocks), dim3(256), 0, st, a);
            else if (nt2 == 2)
                hipLaunchKernelGGL((k_greedy<S1, NT, 2>), dim3(blocks), dim3(256), 0, st, a);
            else if (nt2 == 4 || nt2 == 8)
                hipLaunchKernelGGL((k_greedy<S1, NT, 8>), dim3(blocks), dim3(256), 0, st, a);
            else
                return hipErrorInvalidValue;
            return hipGetLastError();
        } else {
            return hipErrorInvalidValue;
        }
    }
    if (a.common) {
        const unsigned blocks = greedy_common_blocks(a, kGreedyCommonWaves);
        if (a.owner)
            hipLaunchKernelGGL((k_greedy_common<S1, NT, true>), dim3(blocks), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL((k_greedy_common<S1, NT, false>), dim3(blocks), dim3(256), 0, st, a);
        return hipGetLastError();
    }
    const unsigned blocks = greedy_tile_blocks(a, kGreedyWaves);
    hipLaunchKernelGGL((k_greedy<S1, NT, 0>), dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int S1>
static hipError_t dispatch_greedy_s(GreedyArgs& a, hipStream_t st) {
    switch (nt_bucket(a.n1.n_actions)) {
        case 1: return launch_greedy_t<S1, 1>(a, st);
        case 2: return launch_greedy_t<S1, 2>(a, st);
        case 4: return launch_greedy_t<S1, 4>(a, st);
        case 8: return launch_greedy_t<S1, 8>(a, st);
    }
    return hipErrorInvalidValue;
}

hipError_t dispatch_greedy(GreedyArgs& a, hipStream_t st) {
    if (a.E < 1 || (long long)a.E * a.U > 0x7fffffffll || !greedy_fits(a)) return hipErrorInvalidValue;
    if (a.n2.n_groups > 0 &&
        (a.n2.in_dim != 4 || a.n2.hidden != 16 || a.n2.n_actions < 1 || a.n2.n_actions > 128 ||
         a.n2.n_groups != a.n1.n_groups || 2 * a.n_cores + 2 > a.stride || a.n1.n_actions > a.n_cores + 1))
        return hipErrorInvalidValue;
    if (a.owner && (!a.common || a.n_cores < 1 || a.U % a.n_cores != 0)) return hipErrorInvalidValue;
    switch (s1_bucket(a.stride)) {
        case 1: return dispatch_greedy_s<1>(a, st);
        case 2: return dispatch_greedy_s<2>(a, st);
        case 4: return dispatch_greedy_s<4>(a, st);
        case 8: return dispatch_greedy_s<8>(a, st);
    }
    return hipErrorInvalidValue;
}

// both halves of a round in one launch where their shapes have a paired kernel (the shapes k_act_pair is
// built for: cfg2, cfg3, cfg4), else the two launches in order
hipError_t launch_act_round_greedy(GreedyArgs& o, GreedyArgs& c, hipStream_t st) {
    if (o.E < 1 || c.E != o.E || (long long)o.E * o.U > 0x7fffffffll || (long long)c.E * c.U > 0x7fffffffll)
        return hipErrorInvalidValue;
    if (!c.common || !c.owner) return hipErrorInvalidValue;
    const bool price = o.n2.n_groups > 0;
    const int s1a = s1_bucket(o.stride), nta = nt_bucket(o.n1.n_actions);
    const int nt2 = price ? nt_bucket(o.n2.n_actions) : 0;
    const int s1b = s1_bucket(c.stride), ntb = nt_bucket(c.n1.n_actions);
    const int shape = s1a == 1 && nta == 1 && nt2 == 0 && s1b == 1 && ntb == 1   ? 2
                      : s1a == 1 && nta == 1 && nt2 == 1 && s1b == 2 && ntb <= 2 ? 3
                      : s1a == 2 && nta <= 2 && nt2 == 1 && s1b == 4 && ntb <= 4 ? 4
                                                                                 : 0;
    if (!shape) {
        hipError_t e = dispatch_greedy(o, st);
        return e != hipSuccess ? e : dispatch_greedy(c, st);
    }
    // the checks dispatch_greedy makes for each half
    if (!greedy_fits(o) || !greedy_fits(c) || c.n_cores < 1 || c.U % c.n_cores != 0) return hipErrorInvalidValue;
    if (price && (o.n2.in_dim != 4 || o.n2.hidden != 16 || o.n2.n_actions < 1 || o.n2.n_groups != o.n1.n_groups ||
                  2 * o.n_cores + 2 > o.stride || o.n1.n_actions > o.n_cores + 1))
        return hipErrorInvalidValue;
    const unsigned ob = greedy_tile_blocks(o, kGreedyWaves), cb = greedy_common_blocks(c, kGreedyCommonWaves);
    if (shape == 2)
        hipLaunchKernelGGL((k_greedy_pair<1, 1, 0, 1, 1>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
    else if (shape == 3)
        hipLaunchKernelGGL((k_greedy_pair<1, 1, 1, 2, 2>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
    else
        hipLaunchKernelGGL((k_greedy_pair<2, 2, 1, 4, 4>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
    return hipGetLastError();
}

}  // namespace ms

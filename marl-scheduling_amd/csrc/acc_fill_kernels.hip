// acc_fill_kernels.hip — the acceptor items the free-price one-launch rollout leaves (cores their agent does not
// own), sampled from the agents' common-row tables after the launch. No env round here: the tables and the draws
// are the act kernels' (ms_act.h).
#include <hip/hip_runtime.h>

#include "ms_layout.h"
#include "ms_env_launch.h"  // env_rollout_free_supported
#include "ms_act.h"

#pragma clang fp contract(off)  // as the env units (build.sh: -ffp-contract=off)

namespace ms {

// The acceptor items the one-launch rollout leaves (ms_env_rollout_act_free; k_env_rollout_act_free acts with
// act_free<SH, false>): for every acting round t and every (replica e, agent a, core c) whose core a does not own,
// k_act_common's sample from agent a's common-row table (Head::table, ms_act_prepare) with the item's uniform,
// word (i >> 6) & 1 of the draw countered by the row of item i & ~64 (i = e * C + c): the outputs
// ms_act_round_free writes for those items, bit for bit. One thread per item, lanes along the [E][N*C] rows
// (coalesced byte / f32 stores), rounds on blockIdx.y; the N tables in LDS once per block.
struct CommonFillArgs {
    const int8_t* owner;     // round 0's owners [E][C] (the observation the acting of ring slot 1 read)
    int8_t* action;          // round 0's outputs [E][N*C]
    float* logprob;
    int64_t owner_stride, action_stride, logprob_stride;  // bytes per round
    const int8_t* own_action;  // round 0's owned items by core [E][C] (NULL: already in action / logprob)
    const float* own_logprob;
    int64_t own_action_stride, own_logprob_stride;
    const uint32_t* frag;    // the acceptor net's act fragment groups (frag_groups<2, 2>)
    int E, N, C, A;
    uint32_t row_base;
    uint64_t seed, offset, offset_step;
    const uint64_t* offset_dev;
};
constexpr int kFillPer = 8;  // items per thread of k_acc_common_fill: their owner loads in flight together
__global__ void __launch_bounds__(256) k_acc_common_fill(CommonFillArgs p) {
    __shared__ float tabs[8 * kFreeTabDw];
    using FL = FragLayout<2, 2>;
    const int t = blockIdx.y;
    for (int k = threadIdx.x; k < p.N * kFreeTabDw; k += blockDim.x) {
        const int a = k / kFreeTabDw;
        tabs[k] = __uint_as_float(p.frag[(size_t)a * FL::GB + 64 * FL::LW + (k - a * kFreeTabDw)]);
    }
    const int C = p.C, U = p.N * C;
    const int64_t n = (int64_t)p.E * U;
    const uint32_t mag_u = magic_div((uint32_t)U), mag_c = magic_div((uint32_t)C);
    const RawBuf own_b(advance(p.owner, t * p.owner_stride), (int64_t)p.E * C);
    const RawBuf act_b(advance(p.action, t * p.action_stride), n), lp_b(advance(p.logprob, t * p.logprob_stride), 4 * n);
    const uint64_t off = p.offset + (uint64_t)t * p.offset_step + (p.offset_dev ? *p.offset_dev : 0ull);
    // item r = e * U + a * C + c (the [E][N*C] output row): block b takes kFillPer * 256 consecutive items
    const uint32_t r0 = (uint32_t)blockIdx.x * (kFillPer * 256) + threadIdx.x;
    int own[kFillPer];
#pragma unroll
    for (int k = 0; k < kFillPer; k++) {
        const uint32_t r = r0 + 256 * k;
        const uint32_t e = U == 1 ? r : __umulhi(r, mag_u);
        const int u = (int)(r - e * (uint32_t)U);
        const int c = u - small_div(u, C) * C;
        own[k] = own_b.ld8s(e * (uint32_t)C + (uint32_t)c);  // (past the end: 0, the item is skipped below)
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kFillPer; k++) {
        const uint32_t r = r0 + 256 * k;
        const uint32_t e = U == 1 ? r : __umulhi(r, mag_u);
        const int u = (int)(r - e * (uint32_t)U);
        const int a = small_div(u, C), c = u - a * C;
        if ((int64_t)r >= n) continue;
        if (own[k] == a + 1) {  // the owner's row: acted in the rollout launch (by core: copied here)
            if (p.own_action) {
                const size_t oc = (size_t)e * C + c;
                act_b.st8(r, advance(p.own_action, t * p.own_action_stride)[oc]);
                lp_b.stf(4 * r, advance(p.own_logprob, t * p.own_logprob_stride)[oc]);
            }
            continue;
        }
        const uint32_t i = e * (uint32_t)C + (uint32_t)c, ib = i & ~64u;
        const uint32_t eb = C == 1 ? ib : __umulhi(ib, mag_c);
        uint32_t w0, w1;
        philox2(eb * (uint32_t)U + (uint32_t)(a * C) + (ib - eb * (uint32_t)C) + p.row_base, off, p.seed, w0, w1);
        const float* tab = tabs + a * kFreeTabDw;
        const float target = u24((i & 64u) ? w1 : w0) * tab[64];
        int cnt = 0;
#pragma unroll
        for (int step = 32; step >= 1; step >>= 1)
            if (cnt + step <= 32 && tab[cnt + step - 1] <= target) cnt += step;
        const int act = cnt >= p.A ? __float_as_int(tab[65]) : cnt;
        act_b.st8(r, act);
        lp_b.stf(4 * r, tab[32 + act]);
    }
}

// k_acc_common_fill for C % 4 == 0 (the shipped shapes): a thread takes 4 consecutive items (one replica, one
// agent, cores c0..c0+3) of kFillRounds rounds, so the items' index math and Philox rows are computed once, the
// owners come as one dword per round (all rounds' loads in flight together), and a quad none of whose cores its
// agent owns is stored as one dword of actions and one 16-byte vector of log-probs (the per-item kernel: a byte
// and a dword store per item, and the tables loaded once per round per block). PAIR (64 % C == 0): items i and
// i ^ 64 take the two words of one draw, and i ^ 64 is the same agent's core c of replica e ^ (64 / C), so the
// thread also takes that replica's quad and each draw is computed once (the Philox rounds are the kernel's
// largest VALU cost: 32-bit multiplies at quarter rate). Same values bit for bit.
constexpr int kFillRounds = 8;
template <bool PAIR>
__global__ void __launch_bounds__(256) k_acc_common_fill4(CommonFillArgs p, int n_acts) {
    __shared__ __align__(16) float tabs[8 * kFreeTabDw];
    using FL = FragLayout<2, 2>;
    for (int k = threadIdx.x; k < p.N * kFreeTabDw; k += blockDim.x) {
        const int a = k / kFreeTabDw;
        tabs[k] = __uint_as_float(p.frag[(size_t)a * FL::GB + 64 * FL::LW + (k - a * kFreeTabDw)]);
    }
    __syncthreads();
    const int C = p.C, U = p.N * C, QR = U >> 2;  // quads per replica row
    const uint32_t g = (uint32_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t pr = __umulhi(g, magic_div((uint32_t)QR)), uq = g - pr * (uint32_t)QR;
    const uint32_t S = PAIR ? 64u / (uint32_t)C : 1u;  // the partner replica's distance
    const uint32_t e0 = PAIR ? (((pr & ~(S - 1u)) << 1) | (pr & (S - 1u))) : pr, e1 = e0 + S;
    if (e0 >= (uint32_t)p.E) return;
    const bool has1 = PAIR && e1 < (uint32_t)p.E;
    const int u = 4 * (int)uq, a = small_div(u, C), c0 = u - a * C;
    uint32_t row[4], hi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {  // item i = e * C + c: its uniform is word (i >> 6) & 1 of row(i & ~64)'s draw
        if constexpr (PAIR) {      // (i & 64 == 0 for replica e0: row(i) is its own)
            row[k] = e0 * (uint32_t)U + (uint32_t)(u + k) + p.row_base;
        } else {
            const uint32_t i = e0 * (uint32_t)C + (uint32_t)(c0 + k), ib = i & ~64u;
            const uint32_t eb = C == 1 ? ib : __umulhi(ib, magic_div((uint32_t)C));
            row[k] = eb * (uint32_t)U + (uint32_t)(a * C) + (ib - eb * (uint32_t)C) + p.row_base;
            hi |= ((i >> 6) & 1u) << k;
        }
    }
    const float* tab = tabs + a * kFreeTabDw;
    const float tmax = tab[64];
    float bm[3];  // the maxima of the first three blocks of 8 running sums
#pragma unroll
    for (int b = 0; b < 3; b++) bm[b] = tab[8 * b + 7];
    const int t0 = (int)blockIdx.y * kFillRounds;
    uint32_t own0[kFillRounds], own1[kFillRounds];
#pragma unroll
    for (int j = 0; j < kFillRounds; j++) {
        const int8_t* ob = advance(p.owner, (int64_t)(t0 + j) * p.owner_stride);
        own0[j] = t0 + j < n_acts ? *reinterpret_cast<const uint32_t*>(ob + (size_t)e0 * C + c0) : 0u;
        own1[j] = has1 && t0 + j < n_acts ? *reinterpret_cast<const uint32_t*>(ob + (size_t)e1 * C + c0) : 0u;
    }
    const uint64_t off0 = p.offset + (p.offset_dev ? *p.offset_dev : 0ull);
    const uint32_t mine = 0x01010101u * (uint32_t)(a + 1);
    auto store = [&](uint32_t e, int t, int owned, uint32_t acts, const float (&lps)[4]) {
        const size_t r = (size_t)e * U + u;
        int8_t* ad = advance(p.action, (int64_t)t * p.action_stride) + r;
        float* ld = advance(p.logprob, (int64_t)t * p.logprob_stride) + r;
        uint32_t a4 = acts;
        float4 l4 = make_float4(lps[0], lps[1], lps[2], lps[3]);
        if (owned != 0) {  // merge the owned items the rollout wrote: whole quads, no partially written lines (the
            // per-item stores left every line partial: 501 -> 425 us per 199-round fill, profiles/r7s)
            // (by core [E][C]: cores c0..c0 + 3 of replica e; else the rings' own quad)
            const size_t oc = (size_t)e * C + c0;
            const uint32_t old_a = p.own_action
                                       ? *reinterpret_cast<const uint32_t*>(advance(p.own_action, (int64_t)t * p.own_action_stride) + oc)
                                       : *reinterpret_cast<const uint32_t*>(ad);
            const float4 old_l = p.own_action
                                     ? *reinterpret_cast<const float4*>(advance(p.own_logprob, (int64_t)t * p.own_logprob_stride) + oc)
                                     : *reinterpret_cast<const float4*>(ld);
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) m |= ((owned >> k) & 1) ? 0xffu << (8 * k) : 0u;
            a4 = (acts & ~m) | (old_a & m);
            if (owned & 1) l4.x = old_l.x;
            if (owned & 2) l4.y = old_l.y;
            if (owned & 4) l4.z = old_l.z;
            if (owned & 8) l4.w = old_l.w;
        }
        *reinterpret_cast<uint32_t*>(ad) = a4;
        *reinterpret_cast<float4*>(ld) = l4;
    };
#pragma unroll
    for (int j = 0; j < kFillRounds; j++) {
        const int t = t0 + j;
        if (t >= n_acts) break;
        const uint64_t off = off0 + (uint64_t)t * p.offset_step;
        // byte k == 0: the agent owns core c0 + k (acted in the rollout launch); replica e1 absent: all owned
        const uint32_t x0 = own0[j] ^ mine, x1 = has1 ? own1[j] ^ mine : 0u;
        int owned0 = 0, owned1 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            owned0 |= ((x0 >> (8 * k)) & 0xffu) == 0u ? 1 << k : 0;
            owned1 |= ((x1 >> (8 * k)) & 0xffu) == 0u ? 1 << k : 0;
        }
        // every item's draw and search, owned or not (the owned ones are replaced at the store), branch-free and
        // in lockstep: the NI searches' dependent LDS reads of one step issue together instead of one search
        // after the other behind the ownership branches (the kernel is bound by that latency, not by its stores)
        constexpr int NI = PAIR ? 8 : 4;
        float tg[NI];
        int cnt[NI];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t w0, w1;
            philox2(row[k], off, p.seed, w0, w1);
            tg[k] = u24(PAIR ? w0 : (((hi >> k) & 1u) ? w1 : w0)) * tmax;
            if constexpr (PAIR) tg[4 + k] = u24(w1) * tmax;
        }
        // the count of running sums <= target (the binary search's result: the sums are non-decreasing) in two
        // levels: the block of 8 from the 4 block maxima held in registers, then that block's 8 sums (two 16-byte
        // LDS reads, every item's issued together) -- instead of 6 dependent LDS reads per item
#pragma unroll
        for (int i = 0; i < NI; i++) {
            int nb = 0;
#pragma unroll
            for (int b = 0; b < 3; b++) nb += bm[b] <= tg[i] ? 1 : 0;
            cnt[i] = nb;  // block 0..3 (block 3 also when all of its sums are <= target: its count is then 8)
        }
        float4 blo[NI], bhi[NI];
#pragma unroll
        for (int i = 0; i < NI; i++) {
            blo[i] = *reinterpret_cast<const float4*>(tab + 8 * cnt[i]);
            bhi[i] = *reinterpret_cast<const float4*>(tab + 8 * cnt[i] + 4);
        }
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const float t = tg[i];
            cnt[i] = 8 * cnt[i] + (blo[i].x <= t) + (blo[i].y <= t) + (blo[i].z <= t) + (blo[i].w <= t) + (bhi[i].x <= t) +
                     (bhi[i].y <= t) + (bhi[i].z <= t) + (bhi[i].w <= t);
        }
        const int lnz = __float_as_int(tab[65]);
        uint32_t acts0 = 0, acts1 = 0;
        float lps0[4], lps1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int a0 = cnt[k] >= p.A ? lnz : cnt[k];
            acts0 |= (uint32_t)(uint8_t)a0 << (8 * k);
            lps0[k] = tab[32 + a0];
            if constexpr (PAIR) {
                const int a1 = cnt[4 + k] >= p.A ? lnz : cnt[4 + k];
                acts1 |= (uint32_t)(uint8_t)a1 << (8 * k);
                lps1[k] = tab[32 + a1];
            } else {
                lps1[k] = 0.f;
            }
        }
        store(e0, t, owned0, acts0, lps0);
        if (has1) store(e1, t, owned1, acts1, lps1);
    }
}

// where the fill kernels read the agents' common-row tables in an acceptor act fragment block (FragLayout<2, 2>,
// ms_act_prepare with a common row): agent 0's table and the dwords between two agents' tables. The PPO
// gradient's regenerating scan (ms_ppo_batch regen_frag) stages the same words.
void acc_common_tables(const void* act_frag, const uint32_t** tab0, int* group_dwords) {
    using FL = FragLayout<2, 2>;
    static_assert(FL::TB == kFreeTabDw, "common table size");
    *tab0 = static_cast<const uint32_t*>(act_frag) + 4 + 64 * FL::LW;
    *group_dwords = FL::GB;
}
// the acceptor items of cores their agent does not own, every acting round of a k_env_rollout_act_free launch
// with the same arguments (its outputs' other items are untouched)
hipError_t launch_env_fill_common(const Params& P, int64_t E, const StepIO& io, const FusedActFree& fa,
                                  const RoundStrideFree& st, int n_rounds, int act_last, hipStream_t s) {
    const int n_acts = act_last ? n_rounds : n_rounds - 1;
    if (!env_rollout_free_supported(P) || io.obs_cown == nullptr || fa.acc.act_frag == nullptr) return hipErrorInvalidValue;
    if (n_acts < 1) return hipSuccess;
    const CommonFillArgs c{io.obs_cown, fa.acc_action, fa.acc_logprob, st.obs_cown, st.acc_action, st.acc_logprob,
                           fa.own_action, fa.own_logprob, st.own_action, st.own_logprob,
                           static_cast<const uint32_t*>(fa.acc.act_frag) + 4, (int)E, P.N, P.C, fa.acc.n_actions,
                           (uint32_t)fa.acc.row_base, fa.seed, fa.acc_offset, st.offset_step, fa.offset_dev};
    const int64_t items = E * P.N * P.C;
    // the quad kernel: C % 4 == 0 and every round's owners / actions 4-byte, log-probs 16-byte aligned
    const bool quad = P.C % 4 == 0 &&
                      ((reinterpret_cast<uintptr_t>(c.owner) | (uintptr_t)c.owner_stride) & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(c.action) | (uintptr_t)c.action_stride) & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(c.logprob) | (uintptr_t)c.logprob_stride) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(c.own_action) | (uintptr_t)c.own_action_stride) & 3) == 0 &&
                      ((reinterpret_cast<uintptr_t>(c.own_logprob) | (uintptr_t)c.own_logprob_stride) & 15) == 0;
    if (quad) {
        const unsigned by = (unsigned)((n_acts + kFillRounds - 1) / kFillRounds);
        const int64_t qr = (int64_t)P.N * P.C / 4;
        if (64 % P.C == 0) {  // threads: quads of the replicas e with e & (64 / C) == 0
            const int64_t S = 64 / P.C, pairs = (E + 2 * S - 1) / (2 * S) * S;
            hipLaunchKernelGGL(k_acc_common_fill4<true>, dim3((unsigned)((pairs * qr + 255) / 256), by), dim3(256), 0, s,
                               c, n_acts);
        } else {
            hipLaunchKernelGGL(k_acc_common_fill4<false>, dim3((unsigned)((E * qr + 255) / 256), by), dim3(256), 0, s, c,
                               n_acts);
        }
        return hipGetLastError();
    }
    const unsigned bx = (unsigned)((items + kFillPer * 256 - 1) / (kFillPer * 256));
    hipLaunchKernelGGL(k_acc_common_fill, dim3(bx, (unsigned)n_acts), dim3(256), 0, s, c);
    return hipGetLastError();
}
}  // namespace ms

// ms_act_kernels.h — what the acting translation units share (policy_kernels.hip, act_pair_kernels.hip,
// greedy_kernels.hip): the sampling kernels' two device bodies (act_tiles: k_act's; act_common_rows:
// k_act_common's; k_act_pair runs one of each) and the host-side launch plumbing (shape buckets, wave
// splits, size checks). The kernels themselves are defined once, each in the unit whose compiler flags
// suit it (build.sh); their arguments and launchers are declared in ms_act_args.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdlib.h>

#include "../../include/marlsched.h"
#include "ms_common.h"
#include "ms_act.h"
#include "ms_act_args.h"

#pragma clang fp contract(fast)  // as ms_act.h (build.sh: -ffp-contract=fast for the acting units)

namespace ms {

// Profiling build only (tools/build_act_probe.sh: -DMS_ACT_PROBE): lane 0 of every wave of the paired act
// kernel adds the shader-clock cycles between consecutive marks to a per-(half, phase) counter. The product
// library is built without it and the marks compile to nothing.
#ifdef MS_ACT_PROBE
constexpr int kActProbeWaves = 1 << 14;
// per wave slot [half][wave % kActProbeWaves][phase] (plain stores of lane 0: no shared address, so the
// probe's own writes do not queue behind each other in the memory system), summed on the host. Each unit
// that includes this header counts into its own copy; ms_probe_act_cycles reads the paired kernel's.
static __device__ unsigned long long g_act_cycles[2][kActProbeWaves][16];
static __device__ unsigned long long g_act_waves[2][kActProbeWaves];
#define MS_AMARK(k)                                                    \
    do {                                                               \
        const uint64_t t_now = __builtin_amdgcn_s_memtime();          \
        t_acc[k] += t_now - t_prev;                                    \
        t_prev = t_now;                                                \
    } while (0)
#define MS_APROBE_BEGIN                                                \
    uint64_t t_prev = __builtin_amdgcn_s_memtime();                    \
    uint64_t t_acc[16] = {};
#define MS_APROBE_END(half)                                            \
    if (lane == 0) {                                                   \
        const int slot = (block * 4 + (threadIdx.x >> 6)) % kActProbeWaves; \
        for (int k = 0; k < 16; k++) g_act_cycles[half][slot][k] += t_acc[k]; \
        g_act_waves[half][slot] += 1ull;                               \
    }
#else
#define MS_AMARK(k) \
    do {            \
    } while (0)
#define MS_APROBE_BEGIN
#define MS_APROBE_END(half)
#endif

// floats per price-table entry: running sums and log-probs of 16 * NT2 actions, S, last nonzero
template <int NT2>
struct PriceTW {
    static constexpr int v = 32 * NT2 + 4;
};

// One wave = a contiguous range of 16-row tiles of one group; no LDS. Layer 1 runs on the bf16 MFMA
// with the weights split in three bf16 terms (exact f32 weights; the int8 inputs are exact in bf16):
// lane (j, g) loads dwords 8s + 2g, 8s + 2g + 1 of tile row j, which are exactly its B fragment of
// k-step s. S1 = ceil(stride / 32) k-steps.
// (ZFIX: Head's; k_act's instantiations take it, k_act_pair's do not)
template <int S1, int NT, int NT2, bool EXT_U, bool ZFIX = false>
__device__ __forceinline__ void act_tiles(const ActArgs& a, int block) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int gw = block * 4 + __builtin_amdgcn_readfirstlane(tid >> 6);  // global wave index (wave-uniform)
    const int grp = gw / a.waves_per_group;
    const int wv = gw - grp * a.waves_per_group;
    if (grp >= a.n1.n_groups) return;
    MS_APROBE_BEGIN
    const int j = lane & 15, g4 = lane >> 4;
    constexpr int NP = NT2 > 0 ? NT2 : 1;
    constexpr int TW = PriceTW<NP>::v;
    // the arrays this wave touches as raw buffers (32-bit offsets: row indices < 2^24 and arrays
    // < 2^31 bytes, checked at the launch)
    const long long n_rows = (long long)a.E * a.U;
    const long long n_pc = a.pus ? (long long)a.U * a.pus : n_rows;  // price chooser rows
    const RawBuf obs_b(a.obs, n_rows * a.stride), act_b(a.action, n_rows), lp_b(a.logprob, 4 * n_rows);
    const RawBuf pst_b(a.price_state, 4 * n_pc), pact_b(a.price_action, n_pc), plp_b(a.price_logprob, 4 * n_pc),
        envp_b(a.env_price, n_rows);
    const RawBuf tab_b(a.ptab ? a.ptab + (size_t)grp * a.pkeys * TW : nullptr, 4ll * a.pkeys * TW);
    // the price table's key digits, this wave's copy in LDS (a lookup per row: no memory round trip)
    int16_t* pdig = nullptr;
    if constexpr (NT2 > 0) {
        __shared__ uint32_t s_pd[4][512];
        const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
        if (a.ptab) {
            const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pdigit);
            uint32_t v[8];
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = src[64 * k + lane];
#pragma unroll
            for (int k = 0; k < 8; k++) s_pd[wid][64 * k + lane] = v[k];
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
        pdig = reinterpret_cast<int16_t*>(s_pd[wid]);
    }
    W1Split<S1> w1;
    Head<NT, ZFIX> h1;
    if (const uint32_t* fg = frag_groups<S1, NT>(a.n1, false)) {  // made once per weight update
        using FL = FragLayout<S1, NT>;
        const uint32_t* lf = fg + (size_t)grp * FL::GB + lane * FL::LW;
        w1.load_frag(lf);
        h1.load_frag(reinterpret_cast<const float*>(lf + 12 * S1));
    } else {
        w1.load(a.n1.w1 + (size_t)grp * 16 * a.n1.in_dim, a.n1.in_dim, j, g4);
        h1.load(a.n1, grp, j, g4);
    }
    const uint64_t off = a.offset + (a.offset_dev ? *a.offset_dev : 0ull);
    const int stride4 = a.stride >> 2;
    const int n_rows_total = a.E * a.U;
    const int tiles = (a.n_items + 15) >> 4;
    const int t0 = wv * a.tiles_per_wave;
    const int t1 = min(t0 + a.tiles_per_wave, tiles);
    // item i of this group -> obs row: e = i / S by a multiply-high with one correction step
    const uint32_t s_magic = 0xffffffffu / (uint32_t)a.S;
    const uint32_t u_magic = 0xffffffffu / (uint32_t)a.U;  // row -> replica (unit-major price outputs)
    auto row_of_lane = [&](int tile, int jj) -> int {
        const int i = tile * 16 + jj;
        if (i >= a.n_items) return -1;
        int e = (int)__umulhi((uint32_t)i, s_magic);
        if ((e + 1) * a.S <= i) e++;
        return e * a.U + grp * a.S + (i - e * a.S);
    };
    auto row_of = [&](int tile) -> int { return row_of_lane(tile, j); };
    // Philox uniforms, computed for 4 tiles at a time: lane (j, g4) draws for row j of tile
    // base + g4 (counter = the obs row index, so the values do not depend on the tiling)
    uint32_t rnd0 = 0, rnd1 = 0, rb0[4] = {0, 0, 0, 0}, rb1[4] = {0, 0, 0, 0};
    // the counter's row is global across launches (ms_mlp_params.row_base: this call's first replica's
    // first row), so a replica draws the same numbers whichever rank or replica split steps it
    const uint32_t rbase = (uint32_t)a.n1.row_base;
    // With a price net the row's two words are its two uniforms. A single net's row takes word
    // (i >> 6) & 1 of the draw countered by the row of item i & ~64: the rule of k_act_common's scan
    // (one draw per two 64-item steps there), so both kernels sample a row alike.
    auto draw4 = [&](int base) {
        if (NT2 > 0) {
            const int r = base + g4 < t1 ? row_of_lane(base + g4, j) : -1;
            philox2((uint32_t)r + rbase, off, a.seed, rnd0, rnd1);
            rows_bcast(rnd1, rb1);
        } else {
            const int i = (base + g4) * 16 + j;
            const int r = base + g4 < t1 ? row_of_lane(0, i & ~64) : -1;
            philox2((uint32_t)r + rbase, off, a.seed, rnd0, rnd1);
            if (i & 64) rnd0 = rnd1;
        }
        rows_bcast(rnd0, rb0);  // tile base + k takes row k's draws
    };
    auto pick4 = [](const uint32_t (&v)[4], int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3])); };
    // Two tiles per step: their MFMA chains, transcendentals and memory round trips interleave (the
    // kernel is latency-bound with a few waves per SIMD), and their cross-lane sums pair up. A lone
    // last tile runs beside an empty partner (rows -1: nothing written).
    const int A1 = a.n1.n_actions;
    // the pair's uniforms (Philox for 4 tiles at a time, or the given ones)
    auto uniforms2 = [&](int tile, const int (&cur)[2], float (&u1)[2], float (&u2)[2]) {
        if (EXT_U) {
#pragma unroll
            for (int i = 0; i < 2; i++) {
                u1[i] = cur[i] >= 0 ? a.uniforms[cur[i]] : 0.f;
                u2[i] = cur[i] >= 0 && NT2 > 0 ? a.uniforms[n_rows_total + cur[i]] : 0.f;
            }
        } else {
            const int k = (tile - t0) & 3;  // 0 or 2
            if (k == 0) draw4(tile);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                u1[i] = u24(pick4(rb0, k + i));
                u2[i] = u24(pick4(rb1, k + i));
            }
        }
    };
    // the core chooser (or the only net) of both tiles (layer 1: W1Split::layer1's k-step, two tiles interleaved)
    auto core2 = [&](const uint32_t (&xd)[2][S1][2], const float (&u1)[2], int (&act)[2], float (&lp)[2]) {
        f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int s = 0; s < S1; s++) {
            u4v x[2];
#pragma unroll
            for (int i = 0; i < 2; i++) x[i] = bytes_to_bf16(xd[i][s][0], xd[i][s][1]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.hi[s], x[i], acc[i]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.mid[s], x[i], acc[i]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.lo[s], x[i], acc[i]);
        }
        h1.run2(acc, A1, g4, u1, act, lp);
    };
    // price chooser input (PPOmodules.py:316-327): lane g4 takes row byte k of
    // [obs[2a], obs[2a+1], obs[-2], obs[-1]] (obs[-2:] = the slot's pair at 2C), or -5 for a = 0; and
    // the byte's offset in the price table's key (-1: not tabulated; rows of an empty tile: 0)
    auto price_in2 = [&](const uint32_t (&xd)[2][S1][2], const int (&cur)[2], const int (&act)[2], int (&pin)[2],
                         int (&dg)[2]) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int k = g4 < 2 ? 2 * act[i] + g4 : 2 * a.n_cores + (g4 - 2);
            const int src = j + 16 * ((k >> 3) & 3), ks = k >> 5, kh = (k >> 2) & 1;
            uint32_t dw = 0;
#pragma unroll
            for (int s = 0; s < S1; s++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t v = (uint32_t)__shfl((int)xd[i][s][h], src);
                    if (s == ks && h == kh) dw = v;
                }
            pin[i] = act[i] == 0 ? -5 : (int)(int8_t)(dw >> (8 * (k & 3)));
            dg[i] = !a.ptab ? -1 : (cur[i] >= 0 ? (int)pdig[g4 * 256 + pin[i] + 128] : 0);
        }
    };
    // the price chooser's outputs of both tiles
    auto price_out2 = [&](const int (&cur)[2], const int (&act)[2], const int (&pin)[2], const int (&pact)[2],
                          const float (&plp)[2]) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            if (cur[i] >= 0) {
                // the price chooser's rollout rows: [E][U], or unit-major (the update reads one unit's
                // rows of every replica, so they lie contiguous)
                uint32_t pc = (uint32_t)cur[i];
                if (a.pus) {
                    int e = (int)__umulhi((uint32_t)cur[i], u_magic);
                    if ((e + 1) * a.U <= cur[i]) e++;
                    pc = (uint32_t)(cur[i] - e * a.U) * (uint32_t)a.pus + (uint32_t)e;
                }
                pst_b.st8(4 * pc + g4, pin[i]);
                if (g4 == 0) {
                    pact_b.st8(pc, pact[i]);
                    plp_b.stf(4 * pc, plp[i]);
                    envp_b.st8((uint32_t)cur[i], act[i] == 0 ? -5 : pact[i]);
                }
            }
        }
    };
    uint32_t pre[2][S1][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int s = 0; s < S1; s++) pre[i][s][0] = pre[i][s][1] = 0u;
    // (load_row: unconditional loads from clamped addresses; the rows past the end are never written)
    auto load_rows = [&](int r, uint32_t (&dst)[S1][2]) {
        load_row<S1>(obs_b, __umul24((uint32_t)(r < 0 ? 0 : r), (uint32_t)a.stride), stride4, g4, dst);
    };
    int row[2];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        row[i] = t0 + i < t1 ? row_of(t0 + i) : -1;
        if (t0 + i < t1) load_rows(row[i], pre[i]);
    }
    bool any_miss = false;  // a pair with a price input outside the table: priced after the loop
    MS_AMARK(0);  // setup: weights / fragments, the price digits, the first rows' loads issued
    for (int tile = t0; tile < t1; tile += 2) {
        uint32_t xd[2][S1][2];
        int cur[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
#pragma unroll
            for (int s = 0; s < S1; s++) xd[i][s][0] = pre[i][s][0], xd[i][s][1] = pre[i][s][1];
            cur[i] = row[i];
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            row[i] = tile + 2 + i < t1 ? row_of(tile + 2 + i) : -1;
            if (tile + 2 + i < t1) load_rows(row[i], pre[i]);
        }
        MS_AMARK(1);  // row indices + the next pair's loads issued
        float u1[2], u2[2];
        uniforms2(tile, cur, u1, u2);
        MS_AMARK(2);  // Philox
        int act[2];
        float lp[2];
        core2(xd, u1, act, lp);
        MS_AMARK(3);  // core chooser (layer 1 waits for this pair's rows)
        if (NT2 > 0) {
            int pin[2], dg[2];
            price_in2(xd, cur, act, pin, dg);
            if (a.ptab && __ballot(dg[0] < 0 || dg[1] < 0) == 0ull) {
                // every row of both tiles is tabulated: sample from the table (Head::run's arithmetic)
                rows_sum2_i(dg[0], dg[1]);
                float cum[2][NP][4], S2[2];
                int lnz[2], cnt[2], pact[2];
                float plp[2];
                uint32_t te[2];  // byte offset of the row's table entry
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    te[i] = __umul24((uint32_t)dg[i], 4u * TW);
#pragma unroll
                    for (int t = 0; t < NP; t++) {
                        const auto c4 = __builtin_amdgcn_raw_buffer_load_b128(tab_b.r, (int)(te[i] + 4 * (16 * t + 4 * g4)), 0, 0);
#pragma unroll
                        for (int q = 0; q < 4; q++) cum[i][t][q] = __uint_as_float(c4[q]);
                    }
                    S2[i] = tab_b.ldf(te[i] + 4 * (32 * NP));
                    lnz[i] = (int)tab_b.ld32(te[i] + 4 * (32 * NP + 1));
                }
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const float target = u2[i] * S2[i];
                    cnt[i] = 0;
#pragma unroll
                    for (int t = 0; t < NP; t++)
#pragma unroll
                        for (int q = 0; q < 4; q++) cnt[i] += (cum[i][t][q] <= target) ? 1 : 0;
                }
                rows_sum2_i(cnt[0], cnt[1]);
                // the chosen action's log-prob straight from its table entry (one load per row)
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    pact[i] = cnt[i] >= a.n2.n_actions ? lnz[i] : cnt[i];
                    plp[i] = tab_b.ldf(te[i] + 4 * (16 * NP + pact[i]));
                }
                price_out2(cur, act, pin, pact, plp);
            } else {
                any_miss = true;
            }
        }
        MS_AMARK(4);  // price chooser: input, table entry, sample, its stores
#pragma unroll
        for (int i = 0; i < 2; i++)
            if (cur[i] >= 0 && g4 == 0) {
                act_b.st8((uint32_t)cur[i], act[i]);
                lp_b.stf(4 * (uint32_t)cur[i], lp[i]);
            }
        MS_AMARK(5);  // core chooser stores
    }
    if (NT2 > 0 && any_miss) {
        // the pairs the table could not serve (or every pair, without a table): the same pairs and
        // draws again, the core chooser recomputed (bit-identical), then the price net itself; its
        // weights take registers only here, after the main loop
        Head<NP, ZFIX> h2;
        h2.load(a.n2, grp, j, g4);
        const float pw1 = a.n2.w1[((size_t)grp * 16 + j) * 4 + g4];  // W1p[j][g4] (K = 4 inputs)
        for (int tile = t0; tile < t1; tile += 2) {
            uint32_t xd[2][S1][2];
            int cur[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                cur[i] = tile + i < t1 ? row_of(tile + i) : -1;
                load_rows(cur[i], xd[i]);
            }
            float u1[2], u2[2];
            uniforms2(tile, cur, u1, u2);
            int act[2], pin[2], dg[2];
            float lp[2];
            core2(xd, u1, act, lp);
            price_in2(xd, cur, act, pin, dg);
            if (a.ptab && __ballot(dg[0] < 0 || dg[1] < 0) == 0ull) continue;  // priced in the main loop
            int pact[2];
            float plp[2];
            f4 acc2[2];
#pragma unroll
            for (int i = 0; i < 2; i++) acc2[i] = mfma4(pw1, (float)pin[i], (f4){0, 0, 0, 0});
            h2.run2(acc2, a.n2.n_actions, g4, u2, pact, plp);
            price_out2(cur, act, pin, pact, plp);
        }
    }
    MS_AMARK(6);  // untabulated price inputs
    MS_APROBE_END(0)
}

// ---------------------------------------------------------------------------
// k_act_common: ActorCritic.act where many rows equal one common row. Acceptor observations are
// mostly the constant row [0, -1, -1, (-2, -2) * O] of a core the agent does not own
// (Agent.py:167-212: no own job, and every offer to the core is addressed to its owner), so the
// network output of those rows is the same: the wave computes the common row's sampling table
// once (Head::table, the exact arithmetic of Head::run) and samples each row equal to it from its
// own uniform with a handful of compares. The other rows are collected in LDS and run through the
// MFMA tiles as in k_act. Outputs are bit-identical to k_act's.
#ifndef MS_COMMON_SEG
#define MS_COMMON_SEG 512
#endif
constexpr int kCommonSeg = MS_COMMON_SEG;  // most rows per wave = capacity of the wave's LDS row list

template <int S1, int NT, bool EXT_U, bool OWN, bool ZFIX = false>
__device__ __forceinline__ void act_common_rows(const ActArgs& a, int block) {
    __shared__ int32_t s_list[4][kCommonSeg];
    __shared__ float s_ulist[4][kCommonSeg];  // the listed rows' uniforms (drawn in the scan)
    __shared__ float s_cum[4][16 * NT], s_lp[4][16 * NT], s_S[4];
    __shared__ int s_lnz[4];
    __shared__ uint32_t s_tmpl[4][8 * S1];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gw = block * 4 + wid;
    const int grp = gw / a.waves_per_group;
    const int wv = gw - grp * a.waves_per_group;
    if (grp >= a.n1.n_groups) return;  // whole waves only: the kernel has no block barrier
    MS_APROBE_BEGIN
    const int j = lane & 15, g4 = lane >> 4;
    const int A = a.n1.n_actions;
    const int stride4 = a.stride >> 2;
    W1Split<S1> w1;
    Head<NT, ZFIX> h1;
    if (const uint32_t* fg = frag_groups<S1, NT>(a.n1, true)) {
        // the weights and the common row's sampling table as ms_act_prepare made them
        using FL = FragLayout<S1, NT>;
        const uint32_t* gb = fg + (size_t)grp * FL::GB;
        w1.load_frag(gb + lane * FL::LW);
        h1.load_frag(reinterpret_cast<const float*>(gb + lane * FL::LW + 12 * S1));
        const uint32_t* tb = gb + 64 * FL::LW;
        for (int k = lane; k < 32 * NT + 2; k += 64) {
            const uint32_t v = tb[k];
            if (k < 16 * NT)
                s_cum[wid][k] = __uint_as_float(v);
            else if (k < 32 * NT)
                s_lp[wid][k - 16 * NT] = __uint_as_float(v);
            else if (k == 32 * NT)
                s_S[wid] = __uint_as_float(v);
            else
                s_lnz[wid] = (int)v;
        }
    } else {
        w1.load(a.n1.w1 + (size_t)grp * 16 * a.n1.in_dim, a.n1.in_dim, j, g4);
        h1.load(a.n1, grp, j, g4);
        common_table<S1, NT>(w1, h1, a.common, stride4, s_tmpl[wid], s_cum[wid], s_lp[wid], &s_S[wid], &s_lnz[wid],
                             lane);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint64_t off = a.offset + (a.offset_dev ? *a.offset_dev : 0ull);
    int32_t* list = s_list[wid];
    float* ulist = s_ulist[wid];
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(a.common);
    const float* cum = s_cum[wid];  // the running sums, non-decreasing (z >= 0): binary-searched in LDS
    constexpr int LPR = S1 <= 2 ? 4 : (S1 <= 4 ? 8 : 16);
    CommonScan<LPR> cs;
    if (!OWN) cs.init(crow, stride4, lane);
    const float S = s_S[wid];
    const int last_nz = s_lnz[wid];
    const uint32_t s_magic = 0xffffffffu / (uint32_t)a.S;
    auto row_of_item = [&](int i) -> int {
        int e = (int)__umulhi((uint32_t)i, s_magic);
        if ((e + 1) * a.S <= i) e++;
        return e * a.U + grp * a.S + (i - e * a.S);
    };
    // the outputs as raw buffers: 32-bit row offsets, no 64-bit address arithmetic per store
    // (act_common_fits: E * U * 4 bytes < 2^31)
    const long long n_rows = (long long)a.E * a.U;
    const RawBuf act_b(a.action, n_rows), lp_b(a.logprob, 4 * n_rows);
    const int i_begin = wv * a.items_per_wave;
    const int i_end = min(i_begin + a.items_per_wave, a.n_items);  // <= kCommonSeg rows
    // Item i's uniform: word (i >> 6) & 1 of the Philox draw countered by the row of item i & ~64, so
    // one draw serves the rows of two 64-item scan steps (the second step reuses the first's other
    // word). A function of the item index alone: the same for any split of the items into waves.
    uint32_t u_other = 0;  // the draw's second word, kept from the first step of the pair
    auto step_uniform = [&](int i0, int row) -> float {  // i0 = the step's first item (multiple of 64)
        if (EXT_U) return a.uniforms[row < 0 ? 0 : row];
        if ((i0 & 64) && i0 > i_begin) return u24(u_other);
        const int ib = (i0 & ~64) + lane;
        uint32_t r0, r1;
        philox2((uint32_t)row_of_item(ib) + (uint32_t)a.n1.row_base, off, a.seed, r0, r1);
        u_other = r1;
        return u24((i0 & 64) ? r1 : r0);
    };
    const uint64_t below = (1ull << lane) - 1ull;
    int n_list = 0;
    // ---- scan (one 64-row step ahead in registers): rows equal to the common row are sampled
    //      from the table, the others listed
    int n_row = 0;
    bool n_in = false;
    // compact rows: the core row of (e, u) and whether agent u / C + 1 owns core u % C
    // (quotients by a multiply-high with one correction step, as row_of_item: no per-row
    // integer-division sequence)
    const uint32_t u_mag = 0xffffffffu / (uint32_t)a.U, c_mag = 0xffffffffu / (uint32_t)a.n_cores;
    auto core_row_of = [&](int row, int& c_out) -> size_t {
        int e = (int)__umulhi((uint32_t)row, u_mag);
        if ((e + 1) * a.U <= row) e++;
        const int u = row - e * a.U;
        int ag = (int)__umulhi((uint32_t)u, c_mag);
        if ((ag + 1) * a.n_cores <= u) ag++;
        c_out = ag;
        return (size_t)e * a.n_cores + (u - ag * a.n_cores);
    };
    auto load_step = [&](int i0) {
        if constexpr (!OWN) {
            cs.load([&](int k) {
                const int i = i0 + k;
                return reinterpret_cast<const uint32_t*>(a.obs + (size_t)(i < i_end ? row_of_item(i) : 0) * a.stride);
            }, lane);
        }
        const int i = i0 + lane;
        n_in = i < i_end;
        n_row = n_in ? row_of_item(i) : 0;
    };
    // one 64-row step: common rows sample from the table, the others are listed
    auto scan_step = [&](int i0, int row, bool in, bool common) {
        // every lane draws (the lanes of listed rows keep theirs for the tile pass: no second draw
        // there, and no lane-group-replicated one)
        MS_AMARK(2);  // (scan bookkeeping)
        const float u = step_uniform(i0, row);
        MS_AMARK(3);  // Philox (every other step)
        if (common) {
            const float target = u * S;
            // the number of running sums <= target (Head::run's count), by binary search
            int cnt = 0;
#pragma unroll
            for (int step = 16 * NT; step >= 1; step >>= 1)
                if (cnt + step <= 16 * NT && cum[cnt + step - 1] <= target) cnt += step;
            const int act = cnt >= A ? last_nz : cnt;
            act_b.st8((uint32_t)row, act);
            lp_b.stf(4 * (uint32_t)row, s_lp[wid][act]);
        }
        const bool other = in && !common;
        const uint64_t m = __ballot(other);
        if (other) {
            list[n_list + __popcll(m & below)] = row;
            ulist[n_list + __popcll(m & below)] = u;
        }
        n_list += __popcll(m);
        MS_AMARK(4);  // table search, stores, row list
    };
    MS_AMARK(0);  // setup: fragments, the common row's table
    if constexpr (OWN) {
        // compact rows: every step's owner byte is loaded up front (one memory round trip per wave)
        constexpr int MS = kCommonSeg / 64;
        int8_t own_st[MS], me_st[MS];
        int row_st[MS];
        // a group of exactly one agent's C acceptors (locally shared: S == C, unit a*C + c): item i of
        // group g is core row i (replica i / C, core i % C) and the agent is g, so the core row and the
        // owner byte need no per-item quotient
        const bool agent_group = a.S == a.n_cores;
        const RawBuf own_b(a.owner, (long long)a.E * a.n_cores);
#pragma unroll
        for (int st = 0; st < MS; st++) {
            const int i = i_begin + 64 * st + lane;
            row_st[st] = i < i_end ? row_of_item(i) : -1;
            if (agent_group) {
                own_st[st] = (int8_t)own_b.ld8s((uint32_t)(i < i_end ? i : 0));
                me_st[st] = (int8_t)(grp + 1);
            } else {
                int ag;
                const size_t cr = core_row_of(row_st[st] < 0 ? 0 : row_st[st], ag);
                own_st[st] = a.owner[cr];
                me_st[st] = (int8_t)(ag + 1);
            }
        }
        MS_AMARK(1);  // owner loads issued
#pragma unroll
        for (int st = 0; st < MS; st++)
            if (i_begin + 64 * st < i_end)
                scan_step(i_begin + 64 * st, row_st[st], row_st[st] >= 0, row_st[st] >= 0 && own_st[st] != me_st[st]);
    } else {
        // (one 64-row step ahead in registers)
        if (i_begin < i_end) load_step(i_begin);
        for (int i0 = i_begin; i0 < i_end; i0 += 64) {
            const int row = n_row;
            const bool in = n_in;
            const bool common = cs.lane_row_common(lane) && in;
            if (i0 + 64 < i_end) load_step(i0 + 64);
            scan_step(i0, row, in, common);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- the listed rows in 16-row MFMA tiles, two tiles per step (k_act's path; the next pair's rows
    //      prefetched, a lone last tile beside an empty partner)
    uint32_t tp[2][S1][2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int s = 0; s < S1; s++) tp[i][s][0] = tp[i][s][1] = 0u;
    int t_row[2] = {-1, -1};
    float t_u[2] = {0.f, 0.f};
    auto load_tile = [&](int i, int t0) {  // tile starting at list entry t0 (< n_list)
        const int k = t0 + j < n_list ? t0 + j : t0;
        t_row[i] = t0 + j < n_list ? list[k] : -1;
        t_u[i] = ulist[k];
        size_t sr = (size_t)list[k];
        if constexpr (OWN) {
            int ag;
            sr = core_row_of(list[k], ag);
        }
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.obs + sr * a.stride);
#pragma unroll
        for (int s = 0; s < S1; s++) {
            const int c0 = 8 * s + 2 * g4;
            tp[i][s][0] = src[c0 < stride4 ? c0 : stride4 - 1];
            tp[i][s][1] = src[c0 + 1 < stride4 ? c0 + 1 : stride4 - 1];
        }
    };
#pragma unroll
    for (int i = 0; i < 2; i++)
        if (16 * i < n_list) load_tile(i, 16 * i);
    MS_AMARK(5);  // list barrier + first tiles' loads issued
    for (int t0 = 0; t0 < n_list; t0 += 32) {
        int row[2];
        float u[2];
        f4 acc[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int s = 0; s < S1; s++) {
            u4v x[2];
#pragma unroll
            for (int i = 0; i < 2; i++) x[i] = bytes_to_bf16(tp[i][s][0], tp[i][s][1]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.hi[s], x[i], acc[i]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.mid[s], x[i], acc[i]);
#pragma unroll
            for (int i = 0; i < 2; i++) acc[i] = mfma_bf16(w1.lo[s], x[i], acc[i]);
        }
#pragma unroll
        for (int i = 0; i < 2; i++) {
            row[i] = t0 + 16 * i < n_list ? t_row[i] : -1;
            u[i] = t_u[i];
            if (t0 + 32 + 16 * i < n_list) load_tile(i, t0 + 32 + 16 * i);
        }
        MS_AMARK(6);  // listed rows: layer 1 (waits for their loads), the next pair's loads issued
        int act[2];
        float lp[2];
        h1.run2(acc, A, g4, u, act, lp);
        MS_AMARK(7);  // listed rows: layers 2-3, softmax, sample
#pragma unroll
        for (int i = 0; i < 2; i++)
            if (row[i] >= 0 && g4 == 0) {
                act_b.st8((uint32_t)row[i], act[i]);
                lp_b.stf(4 * (uint32_t)row[i], lp[i]);
            }
        MS_AMARK(8);  // listed rows' stores
    }
    MS_APROBE_END(1)
}

// launch-shape knobs for measurements (tools/); the defaults are the measured best for cfg3
static long long env_int(const char* name, long long dflt) {
    const char* v = getenv(name);
    return v && *v ? atoll(v) : dflt;
}

// The kernels are built for 1, 2, 4 or 8 layer-1 k-steps (32 row bytes each) and 16-action tiles: the
// bucket a count falls in, 0 beyond 8 (not built)
static int act_bucket(int n) { return n <= 1 ? 1 : (n <= 2 ? 2 : (n <= 4 ? 4 : (n <= 8 ? 8 : 0))); }
static int s1_bucket(int stride) { return act_bucket((stride + 31) / 32); }
static int nt_bucket(int n_actions) { return act_bucket((n_actions + 15) / 16); }

// launch shapes: ~target waves over all groups in blocks of four (set the wave split, return the blocks).
// Tiles: each wave walks a contiguous range of 16-row tiles with a register prefetch.
static unsigned tile_blocks(int n_items, int G, long long target, int* tiles_per_wave, int* waves_per_group) {
    const int tiles = (n_items + 15) / 16;
    const int tpw = (int)(((long long)tiles * G + target - 1) / target);
    *tiles_per_wave = tpw < 1 ? 1 : tpw;
    *waves_per_group = (tiles + *tiles_per_wave - 1) / *tiles_per_wave;
    return (unsigned)(((long long)*waves_per_group * G + 3) / 4);
}
// Common rows: whole scan quanta per wave (quantum items), at most seg_cap (one LDS list of rows).
static unsigned common_blocks(int n_items, int G, long long target, int quantum, int seg_cap, int* items_per_wave,
                              int* waves_per_group) {
    long long ipw = ((long long)n_items * G + target - 1) / target;
    ipw = (ipw + quantum - 1) / quantum * quantum;
    ipw = ipw < quantum ? quantum : (ipw > seg_cap ? seg_cap : ipw);
    *items_per_wave = (int)ipw;
    *waves_per_group = (n_items + *items_per_wave - 1) / *items_per_wave;
    return (unsigned)(((long long)*waves_per_group * G + 3) / 4);
}
static unsigned act_blocks(ActArgs& a, long long target) {
    return tile_blocks(a.n_items, a.n1.n_groups, target, &a.tiles_per_wave, &a.waves_per_group);
}
// (whole step pairs: one Philox draw serves two 64-item scan steps)
static unsigned act_common_blocks(ActArgs& a, long long target) {
    return common_blocks(a.n_items, a.n1.n_groups, target, 128, kCommonSeg, &a.items_per_wave, &a.waves_per_group);
}

// act_common_rows stores through 31-bit byte offsets (RawBuf) and reads compact owners by item index
static bool act_common_fits(const ActArgs& a) {
    return (long long)a.E * a.U * 4 <= 0x7fffffffll && (long long)a.E * (a.n_cores > 0 ? a.n_cores : 1) <= 0x7fffffffll;
}

// act_tiles addresses rows with 24-bit row indices and 31-bit byte offsets (RawBuf)
static bool act_tiles_fits(const ActArgs& a) {
    const long long rows = (long long)a.E * a.U;
    const long long pc = a.pus ? (long long)a.U * a.pus : rows;
    return rows < (1ll << 24) && rows * a.stride <= 0x7fffffffll && 4 * pc <= 0x7fffffffll &&
           (long long)a.pkeys * PriceTW<8>::v * 4 <= 0x7fffffffll;
}

}  // namespace ms

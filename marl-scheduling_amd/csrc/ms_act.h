// ms_act.h — the forward pass of the acting nets, shared by the sampling and greedy act kernels
// (ms_act_kernels.h, policy_kernels.hip, act_pair_kernels.hip, greedy_kernels.hip) and the env round's
// fused acting of fixed-price global nets (ms_env_round.h): Philox2x32 uniforms, the clamped row load,
// the exact three-term bf16 layer 1 (W1Split), the 16-wide head with its logits and its softmax /
// Categorical sampling (Head) and the act fragment block layout (ms_act_prepare).
// PPOmodules.py:53-63 (ActorCritic.act).
//
// Every includer gets the same floating-point contraction here (the policy kernels' -ffp-contract=fast),
// whatever its own flags, so the fused acting of the env kernel (built with contraction off) rounds
// exactly as k_act does. An includer restores its own setting after the include.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/marlsched.h"
#include "ms_common.h"

#pragma clang fp contract(fast)

#include "ms_mfma.h"  // f4 / u4v, mfma4, mfma_bf16, pack_hi, trunc_bf16, bytes_to_bf16, fast_tanh_b, fast_exp, fast_log (under the contraction set above)

namespace ms {

// (mulhilo, philox2 and u24 live in ms_common.h: the PPO gradient regenerates acting draws with them)

// A tile's rows as loaded: lane (j, g4) takes dwords 8s + 2 g4, 8s + 2 g4 + 1 of its row j, exactly its B
// fragment of k-step s. Unconditional loads from clamped addresses, used as loaded: the dwords past the
// row (stride4 dwords) repeat its last one and meet zero weights, so the wait lands at the use.
template <int S1>
__device__ __forceinline__ void load_row(const RawBuf& b, uint32_t row_byte, int stride4, int g4,
                                         uint32_t (&dst)[S1][2]) {
#pragma unroll
    for (int s = 0; s < S1; s++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int cc = 8 * s + 2 * g4 + h;
            dst[s][h] = b.ld32(row_byte + 4 * (cc < stride4 ? cc : stride4 - 1));
        }
}

// Layer-1 weights as three bf16 terms, w = hi + mid + lo exactly (truncation leaves exact residuals),
// in the A-operand layout of v_mfma_f32_16x16x32_bf16 for k-step s: lane (i, g) holds
// W1[i][32s + 8g + 0..7].
template <int S1>
struct W1Split {
    u4v hi[S1], mid[S1], lo[S1];
    // the 12*S1 dwords of a lane's fragment (ms_act_prepare) in the act fragment block
    __device__ __forceinline__ void store_frag(uint32_t* f) const {
#pragma unroll
        for (int s = 0; s < S1; s++) {
            *reinterpret_cast<u4v*>(f + 12 * s) = hi[s];
            *reinterpret_cast<u4v*>(f + 12 * s + 4) = mid[s];
            *reinterpret_cast<u4v*>(f + 12 * s + 8) = lo[s];
        }
    }
    __device__ __forceinline__ void load_frag(const uint32_t* f) {
#pragma unroll
        for (int s = 0; s < S1; s++) {
            hi[s] = *reinterpret_cast<const u4v*>(f + 12 * s);
            mid[s] = *reinterpret_cast<const u4v*>(f + 12 * s + 4);
            lo[s] = *reinterpret_cast<const u4v*>(f + 12 * s + 8);
        }
    }
    // Layer 1 of one tile (pre-activations without the bias) from its rows as load_row leaves them: per
    // k-step the three terms' MFMAs, hi, mid, lo. The sampling kernels spell the same sequence out where
    // they interleave two tiles or read the row from LDS (act_tiles, act_common_rows, common_table, the env
    // round's fused acting): through this helper their register allocation changes.
    __device__ __forceinline__ f4 layer1(const uint32_t (&xd)[S1][2]) const {
        f4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < S1; s++) {
            const u4v x = bytes_to_bf16(xd[s][0], xd[s][1]);
            acc = mfma_bf16(hi[s], x, acc);
            acc = mfma_bf16(mid[s], x, acc);
            acc = mfma_bf16(lo[s], x, acc);
        }
        return acc;
    }
    __device__ void load(const float* w1 /* [16][D] of this group */, int D, int i, int g) {
#pragma unroll
        for (int s = 0; s < S1; s++) {
            float h[8], m[8], l[8];
#pragma unroll
            for (int e = 0; e < 8; e++) {
                const int k = 32 * s + 8 * g + e;
                const float w = k < D ? w1[i * D + k] : 0.f;
                h[e] = trunc_bf16(w);
                const float r1 = w - h[e];
                m[e] = trunc_bf16(r1);
                l[e] = r1 - m[e];  // <= 8 significant bits: exact in bf16
            }
#pragma unroll
            for (int d = 0; d < 4; d++) {
                hi[s][d] = pack_hi(h[2 * d], h[2 * d + 1]);
                mid[s][d] = pack_hi(m[2 * d], m[2 * d + 1]);
                lo[s][d] = pack_hi(l[2 * d], l[2 * d + 1]);
            }
        }
    }
};

// The 16-wide layers and the head of one net, in registers: lane (j, g4) holds W2[j][4*g4 + s],
// W3[16t + j][4*g4 + s] (the permuted-k A operands) and the biases of its accumulator rows.
// ZFIX: the sampling never lands on an action whose numerator is exactly 0 (run2's second look, the tables'
// zero entries: numerators()). The single launches and the table builders of policy_kernels.hip take it;
// k_act_pair and the env round's fused acting keep the plain count (their code is the benchmark's, and the
// check cost 1.3 to 3.3 % of a cfg3 step in either form tried: profiles/r14_act_buckets), so only the rows
// they compute themselves, not the ones they sample from a table, can still meet the one-rounding-step
// window described at run2.
template <int NT, bool ZFIX = false>
struct Head {
    float b1[4], w2[4], b2[4], w3[NT][4], b3[NT][4];  // b1, b2 pre-scaled by kTanhScale (fast_tanh_b)
    static constexpr int FW = 12 + 8 * NT;  // dwords of a lane's fragment
    __device__ __forceinline__ void store_frag(float* f) const {
#pragma unroll
        for (int q = 0; q < 4; q++) {
            f[q] = b1[q];
            f[4 + q] = w2[q];
            f[8 + q] = b2[q];
#pragma unroll
            for (int t = 0; t < NT; t++) {
                f[12 + 4 * t + q] = w3[t][q];
                f[12 + 4 * NT + 4 * t + q] = b3[t][q];
            }
        }
    }
    __device__ __forceinline__ void load_frag(const float* f) {
#pragma unroll
        for (int q4 = 0; q4 < 3 + 2 * NT; q4++) {
            const f4 v = *reinterpret_cast<const f4*>(f + 4 * q4);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float x = v[q];
                if (q4 == 0) b1[q] = x;
                else if (q4 == 1) w2[q] = x;
                else if (q4 == 2) b2[q] = x;
                else if (q4 < 3 + NT) w3[q4 - 3][q] = x;
                else b3[q4 - 3 - NT][q] = x;
            }
        }
    }
    __device__ void load(const ms_mlp_params& p, int grp, int j, int g4) {
        const int A = p.n_actions;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            b1[q] = p.b1[grp * 16 + 4 * g4 + q] * kTanhScale;
            w2[q] = p.w2[(size_t)grp * 256 + j * 16 + 4 * g4 + q];
            b2[q] = p.b2[grp * 16 + 4 * g4 + q] * kTanhScale;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                const int a = 16 * t + j, ab = 16 * t + 4 * g4 + q;
                w3[t][q] = a < A ? p.w3[((size_t)grp * A + a) * 16 + 4 * g4 + q] : 0.f;
                b3[t][q] = ab < A ? p.b3[(size_t)grp * A + ab] : -INFINITY;  // padding actions: exp -> 0
            }
        }
    }

    // Layers 2-3 of the 16 rows of a tile given layer-1 pre-activations: z[t][q] = the logit of action
    // a = 16t + 4*g4 + q of row j. Logits of the padding actions (a >= A) read -inf (bias). Returns the
    // largest of this lane's logits (what a softmax needs next; folded in as each logit is formed).
    __device__ __forceinline__ float logits(f4 a1, float (&z)[NT][4]) const {
        return logits(a1, z, [](int, int, float v) { return v; });
    }
    // (fix(t, q, logit) replaces each logit as it is formed: the greedy kernels' mask by action index)
    template <class F>
    __device__ __forceinline__ float logits(f4 a1, float (&z)[NT][4], F fix) const {
        float h1[4];
#pragma unroll
        for (int q = 0; q < 4; q++) h1[q] = fast_tanh_b(a1[q], b1[q]);
        f4 a2 = {0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 4; s++) a2 = mfma4(w2[s], h1[s], a2);
        float h2[4];
#pragma unroll
        for (int q = 0; q < 4; q++) h2[q] = fast_tanh_b(a2[q], b2[q]);
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            f4 zz = {0, 0, 0, 0};
#pragma unroll
            for (int s = 0; s < 4; s++) zz = mfma4(w3[t][s], h2[s], zz);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                z[t][q] = fix(t, q, zz[q] + b3[t][q]);
                m = fmaxf(m, z[t][q]);
            }
        }
        return m;
    }

    // The softmax numerators of the tile's rows: z[t][q] = exp(logit - max) of action a = 16t + 4*g4 + q
    // of row j, S = the row's sum of z and c[t][q] = the running sum of z over actions 0..a (in increasing
    // action order; with ZFIX an action with a zero numerator: the running sum of the last nonzero action
    // before it, 0 when there is none). The padding actions' -inf logits drop out of the max and the sums.
    __device__ __forceinline__ void numerators(f4 a1, int g4, float (&z)[NT][4], float (&c)[NT][4], float& S) const {
        float m = logits(a1, z);
        m = rows_max(m);
        float bs[NT];
        const float m_l2e = m * 1.4426950408889634f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            bs[t] = 0.f;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                z[t][q] = fast_exp_sub(z[t][q], m_l2e);
                bs[t] += z[t][q];
            }
        }
        float lane_tot = 0.f;
#pragma unroll
        for (int t = 0; t < NT; t++) lane_tot += bs[t];
        // (one 16-action tile: S is the running sums' total, (gs0 + gs1) + (gs2 + gs3), which is
        //  rows_sum(lane_tot) bit for bit)
        if (NT > 1) S = rows_sum(lane_tot);
        float cum = 0.f;
        [[maybe_unused]] float live_c = 0.f;  // ZFIX: the running sum of the last nonzero action so far (0: none)
#pragma unroll
        for (int t = 0; t < NT; t++) {
            uint32_t gsr[4];
            rows_bcast(__float_as_uint(bs[t]), gsr);
            const float gs0 = __uint_as_float(gsr[0]), gs1 = __uint_as_float(gsr[1]), gs2 = __uint_as_float(gsr[2]),
                        gs3 = __uint_as_float(gsr[3]);
            float cc = cum + (g4 > 0 ? gs0 : 0.f) + (g4 > 1 ? gs1 : 0.f) + (g4 > 2 ? gs2 : 0.f);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                cc += z[t][q];
                c[t][q] = cc;
            }
            cum += (gs0 + gs1) + (gs2 + gs3);
            if constexpr (ZFIX) {
                // A zero numerator takes the running sum of the last nonzero action before it, to the bit: the
                // lanes and tiles add their sums in different orders, so its own sum can sit one rounding step
                // above that one, and a u * S between the two would count up to the zero-probability action.
                // With equal sums the count passes over it (or reaches the padding: last nonzero).
                float mine_c = 0.f;  // the running sum of this lane's last nonzero action of the tile
#pragma unroll
                for (int q = 0; q < 4; q++) mine_c = z[t][q] > 0.f ? c[t][q] : mine_c;
                uint32_t er[4];
                rows_bcast(__float_as_uint(mine_c), er);
                float prev = live_c;
                if (g4 > 0 && gs0 > 0.f) prev = __uint_as_float(er[0]);
                if (g4 > 1 && gs1 > 0.f) prev = __uint_as_float(er[1]);
                if (g4 > 2 && gs2 > 0.f) prev = __uint_as_float(er[2]);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    if (z[t][q] > 0.f)
                        prev = c[t][q];
                    else
                        c[t][q] = prev;
                }
                if (gs0 > 0.f) live_c = __uint_as_float(er[0]);
                if (gs1 > 0.f) live_c = __uint_as_float(er[1]);
                if (gs2 > 0.f) live_c = __uint_as_float(er[2]);
                if (gs3 > 0.f) live_c = __uint_as_float(er[3]);
            }
        }
        if (NT == 1) S = cum;
    }

    // run() of two tiles side by side: their MFMA chains and transcendentals interleave, and their
    // cross-lane reductions pair up (rows_max2, rows_sum2, rows_sum2_i). The running sums are compared
    // with u * S as they are formed instead of being kept. Bit-identical to two run() calls.
    __device__ __forceinline__ void run2(const f4 (&a1)[2], int A, int g4, const float (&u)[2], int (&action)[2],
                                         float (&logprob)[2]) const {
        float h1[2][4];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int q = 0; q < 4; q++) h1[i][q] = fast_tanh_b(a1[i][q], b1[q]);
        f4 a2[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int i = 0; i < 2; i++) a2[i] = mfma4(w2[s], h1[i][s], a2[i]);
        float h2[2][4];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int q = 0; q < 4; q++) h2[i][q] = fast_tanh_b(a2[i][q], b2[q]);
        float z[2][NT][4];
        float m[2] = {-INFINITY, -INFINITY};
#pragma unroll
        for (int t = 0; t < NT; t++) {
            f4 zz[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
            for (int s = 0; s < 4; s++)
#pragma unroll
                for (int i = 0; i < 2; i++) zz[i] = mfma4(w3[t][s], h2[i][s], zz[i]);
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    z[i][t][q] = zz[i][q] + b3[t][q];
                    m[i] = fmaxf(m[i], z[i][t][q]);
                }
        }
        rows_max2(m[0], m[1]);
        float bs[2][NT], S[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float m_l2e = m[i] * 1.4426950408889634f;
            S[i] = 0.f;
#pragma unroll
            for (int t = 0; t < NT; t++) {
                bs[i][t] = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    z[i][t][q] = fast_exp_sub(z[i][t][q], m_l2e);
                    bs[i][t] += z[i][t][q];
                }
            }
#pragma unroll
            for (int t = 0; t < NT; t++) S[i] += bs[i][t];
        }
        int cnt[2];
        if (NT > 1) {
            rows_sum2(S[0], S[1]);  // = rows_sum(lane_tot) of numerators()
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const float target = u[i] * S[i];
                float cum = 0.f;
                cnt[i] = 0;
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    uint32_t gsr[4];
                    rows_bcast(__float_as_uint(bs[i][t]), gsr);
                    const float gs0 = __uint_as_float(gsr[0]), gs1 = __uint_as_float(gsr[1]),
                                gs2 = __uint_as_float(gsr[2]), gs3 = __uint_as_float(gsr[3]);
                    float cc = cum + (g4 > 0 ? gs0 : 0.f) + (g4 > 1 ? gs1 : 0.f) + (g4 > 2 ? gs2 : 0.f);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        cc += z[i][t][q];
                        cnt[i] += (cc <= target) ? 1 : 0;
                    }
                    cum += (gs0 + gs1) + (gs2 + gs3);
                }
            }
        } else {
            // one 16-action tile: S is the running sums' total (gs0 + gs1) + (gs2 + gs3), known only
            // after the broadcast, so the running sums are kept for the compare
            float c[2][4];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                uint32_t gsr[4];
                rows_bcast(__float_as_uint(bs[i][0]), gsr);
                const float gs0 = __uint_as_float(gsr[0]), gs1 = __uint_as_float(gsr[1]), gs2 = __uint_as_float(gsr[2]),
                            gs3 = __uint_as_float(gsr[3]);
                const float cum = 0.f;  // numerators()' expression, term for term
                float cc = cum + (g4 > 0 ? gs0 : 0.f) + (g4 > 1 ? gs1 : 0.f) + (g4 > 2 ? gs2 : 0.f);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    cc += z[i][0][q];
                    c[i][q] = cc;
                }
                S[i] = cum + ((gs0 + gs1) + (gs2 + gs3));
                const float target = u[i] * S[i];
                cnt[i] = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) cnt[i] += (c[i][q] <= target) ? 1 : 0;
            }
        }
        rows_sum2_i(cnt[0], cnt[1]);
        if (__builtin_expect(__ballot(cnt[0] >= A || cnt[1] >= A) != 0, 0)) {
            // u * S at or beyond the rounded total: the last action with nonzero probability
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int last_nz = last_nonzero(z[i], g4);
                if (cnt[i] >= A) cnt[i] = last_nz;
            }
        }
        float mine[2] = {0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) mine[i] = (16 * t + 4 * g4 + q == cnt[i]) ? z[i][t][q] : mine[i];
        if constexpr (ZFIX) {
            // The count stopped on a zero numerator (this lane holds that action): the lanes and tiles add
            // their running sums in different orders, so the sum of the last nonzero action can sit one
            // rounding step below the next lane's, with u * S between the two. A zero-probability action is
            // never drawn: the last action with nonzero probability before the count (the tables give their
            // zero numerators that action's running sum: numerators()).
            bool off[2];
#pragma unroll
            for (int i = 0; i < 2; i++) off[i] = ((cnt[i] >> 2) & 3) == g4 && mine[i] == 0.f;
            if (__builtin_expect(__ballot(off[0] || off[1]) != 0, 0)) {
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const int row_off = rows_max_i(off[i] ? 1 : 0);
                    const int last_nz = last_nonzero_below(z[i], g4, cnt[i]);
                    if (row_off && last_nz >= 0) cnt[i] = last_nz;
                    mine[i] = 0.f;
                }
#pragma unroll
                for (int i = 0; i < 2; i++)
#pragma unroll
                    for (int t = 0; t < NT; t++)
#pragma unroll
                        for (int q = 0; q < 4; q++) mine[i] = (16 * t + 4 * g4 + q == cnt[i]) ? z[i][t][q] : mine[i];
            }
        }
        rows_sum2(mine[0], mine[1]);
#pragma unroll
        for (int i = 0; i < 2; i++) {
            action[i] = cnt[i];
            logprob[i] = clamped_log(mine[i] * __builtin_amdgcn_rcpf(S[i]));
        }
    }

    __device__ __forceinline__ static int last_nonzero(const float (&z)[NT][4], int g4) {
        int last_nz = -1;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (z[t][q] > 0.f) last_nz = 16 * t + 4 * g4 + q;
        last_nz = rows_max_i(last_nz);
        return last_nz;
    }
    // the row's last action below `below` with a nonzero numerator (-1: none), on every lane of the row
    __device__ __forceinline__ static int last_nonzero_below(const float (&z)[NT][4], int g4, int below) {
        int last_nz = -1;
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (z[t][q] > 0.f && 16 * t + 4 * g4 + q < below) last_nz = 16 * t + 4 * g4 + q;
        return rows_max_i(last_nz);
    }

    __device__ __forceinline__ static float clamped_log(float pa) {
        const float eps = 1.1920928955078125e-07f;  // torch.finfo(float32).eps
        return fast_log(fminf(fmaxf(pa, eps), 1.f - eps));
    }

    // The sampling entries of the tile's 16 rows, one row per column j: lane (j, g4) gets its four
    // actions' running sums c and log-probs lp (what run() would compare and return), and S and the
    // last nonzero action of row j (every lane of the row).
    __device__ __forceinline__ void row_table(f4 a1, int g4, float (&c)[NT][4], float (&lp)[NT][4], float& S,
                                              int& last_nz) const {
        float z[NT][4];
        numerators(a1, g4, z, c, S);
        last_nz = last_nonzero(z, g4);
        const float rS = __builtin_amdgcn_rcpf(S);
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) lp[t][q] = clamped_log(z[t][q] * rS);
    }

    // The sampling table of one row (all 16 rows of the tile equal): cum[a] = running sum through
    // action a, lp[a] = the log-prob run() returns for action a, *S and *last_nz. With it, a row equal
    // to this one samples and scores exactly as run() would.
    __device__ __forceinline__ void table(f4 a1, int j, int g4, float* cum, float* lp, float* S_out,
                                          int* last_nz_out) const {
        float z[NT][4], c[NT][4], S;
        numerators(a1, g4, z, c, S);
        const int last_nz = last_nonzero(z, g4);
        if (j == 0) {
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int a = 16 * t + 4 * g4 + q;
                    cum[a] = c[t][q];
                    lp[a] = clamped_log(z[t][q] * __builtin_amdgcn_rcpf(S));
                }
            if (g4 == 0) {
                *S_out = S;
                *last_nz_out = last_nz;
            }
        }
    }
};

// ---- act fragment block (ms_act_prepare): a header {magic, S1, NT, has common table}, then per group
//      [64 lanes][LW] dwords (the lane's W1Split<S1> terms and Head<NT> parameters, exactly what the
//      acting wave would derive) and the common row's sampling table [16 NT running sums][16 NT
//      log-probs][S][last nonzero][2 pad] (Head::table)
constexpr uint32_t kFragMagic = 0x4D534641u;
template <int S1, int NT>
struct FragLayout {
    static constexpr int LW = 12 * S1 + Head<NT>::FW;  // dwords per lane (a multiple of 4)
    static constexpr int TB = 32 * NT + 4;              // common table dwords
    static constexpr int GB = 64 * LW + TB;             // dwords per group
};
// the group blocks of p's fragment block, or NULL when it is absent or made for another shape
template <int S1, int NT>
__device__ __forceinline__ const uint32_t* frag_groups(const ms_mlp_params& p, bool need_common) {
    const uint32_t* f = static_cast<const uint32_t*>(p.act_frag);
    if (!f) return nullptr;
    const uint32_t h0 = __builtin_amdgcn_readfirstlane(f[0]), h1 = __builtin_amdgcn_readfirstlane(f[1]),
                   h2 = __builtin_amdgcn_readfirstlane(f[2]), h3 = __builtin_amdgcn_readfirstlane(f[3]);
    if (h0 != kFragMagic || h1 != (uint32_t)S1 || h2 != (uint32_t)NT || (need_common && !h3)) return nullptr;
    return f + 4;
}

// The common row's sampling table (Head::table) into LDS: its dwords (zero past the row: they meet
// zero weights, like k_act's clamped loads) through layer 1 and the head. One wave.
template <int S1, int NT, bool ZFIX>
__device__ __forceinline__ void common_table(const W1Split<S1>& w1, const Head<NT, ZFIX>& h1, const int8_t* common,
                                             int stride4, uint32_t* tmpl, float* cum, float* lp, float* S, int* lnz,
                                             int lane) {
    const int j = lane & 15, g4 = lane >> 4;
    const uint32_t* crow = reinterpret_cast<const uint32_t*>(common);
    for (int d = lane; d < 8 * S1; d += 64) tmpl[d] = d < stride4 ? crow[d] : 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    f4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < S1; s++) {
        const u4v x = bytes_to_bf16(tmpl[8 * s + 2 * g4], tmpl[8 * s + 2 * g4 + 1]);
        acc = mfma_bf16(w1.hi[s], x, acc);
        acc = mfma_bf16(w1.mid[s], x, acc);
        acc = mfma_bf16(w1.lo[s], x, acc);
    }
    h1.table(acc, j, g4, cum, lp, S, lnz);
}

}  // namespace ms

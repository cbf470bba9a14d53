// env_auct_kernels.hip — the fixed-price fused launches with a learned auctioneer (ms_env_step_act_auct,
// ms_env_rollout_act_auct): env_kernels.hip's k_env_step_act and k_env_rollout_act with the round's auctioneer
// actions read from an array (env_round's io.act_auct path: no tie-break draw from the env stream) and the next
// round's acting of a third net, the auctioneer's, after the offer units' and the acceptors'. A unit of its own
// with the round loop written out again: env_kernels.hip's kernels compile to what they did before this unit
// existed (profiles/auct).
#include <hip/hip_runtime.h>

#include "ms_env_auct_launch.h"
#include "ms_env_launch.h"
#include "ms_env_round.h"

namespace ms {

// ---- the auctioneer's next-round acting of the wave's envs: ActorCritic.act of one net on the auctioneer rows
//      (gatherDividedAuctioneerObservation: core row c where nobody owns core c, else the foreign row) from the
//      observations the round left in its LDS, with fused_act's arithmetic for the acceptors: the cores' rows
//      (EPW * C <= 16: one tile) through the net's fragments, of which the unowned cores' items take the result;
//      every other item samples the net's common-row table, one lane per item. Item i = e * C + c, its uniform
//      word (i >> 6) & 1 of the draw countered by (i & ~64) + row_base (k_act_common's rule), so the outputs equal
//      ms_policy_act_compact(core_rows, core_owner == 0, n_units = C) on the emitted rows.
template <int LPE, class SH>
__device__ __forceinline__ void auct_act(const Params& P, int64_t E, const FusedAct& fa, const AuctAct& aa,
                                         int64_t slot, int lane_arg = -1) {
    constexpr int EPW = kWave / LPE;  // envs per wave
    extern __shared__ __align__(16) uint8_t smem_all[];
    __shared__ float s_acum[16], s_alp[16];
    __shared__ uint32_t s_atab[2];  // the common row's S (f32 bits) and last nonzero action
    __shared__ uint32_t s_atmpl[8];
    Geom g;
    if constexpr (SH::kStatic) {
        constexpr Geom kg = make_geom(SH::kN, SH::kC, SH::kL, SH::kJ);
        g = kg;
    } else {
        g = P;
    }
    const int lane = lane_arg >= 0 ? lane_arg : (int)threadIdx.x, j = lane & 15, g4 = lane >> 4;
    const int C = g.C;
    const int64_t e0 = slot * EPW;
    const uint64_t off = aa.offset + (fa.offset_dev ? *fa.offset_dev : 0ull);
    W1Split<1> wa;
    Head<1> ha;
    using FL = FragLayout<1, 1>;
    const uint32_t* fc = frag_groups<1, 1>(aa.net, true);
    if (fc) {
        wa.load_frag(fc + lane * FL::LW);
        ha.load_frag(reinterpret_cast<const float*>(fc + lane * FL::LW + 12));
        if (lane < 34) {
            const uint32_t v = fc[64 * FL::LW + lane];  // [16 running sums][16 log-probs][S][last nonzero]
            if (lane < 16)
                s_acum[lane] = __uint_as_float(v);
            else if (lane < 32)
                s_alp[lane - 16] = __uint_as_float(v);
            else
                s_atab[lane - 32] = v;
        }
    } else {
        wa.load(aa.net.w1, aa.net.in_dim, j, g4);
        ha.load(aa.net, 0, j, g4);
        float S0;
        int lnz0;
        common_table<1, 1>(wa, ha, fa.common, g.acc_stride >> 2, s_atmpl, s_acum, s_alp, &S0, &lnz0, lane);
        if (lane == 0) {
            s_atab[0] = __float_as_uint(S0);
            s_atab[1] = (uint32_t)lnz0;
        }
    }
    wave_sync();
    const int A = aa.net.n_actions, nw = g.acc_stride >> 2;
    auto philox_u = [&](int64_t item) {
        uint32_t r0, r1;
        philox2((uint32_t)(item & ~64ll) + (uint32_t)aa.net.row_base, off, fa.seed, r0, r1);
        return u24((item & 64) ? r1 : r0);
    };
    // ---- the cores nobody owns: row j of the tile is core (ge, c)'s row
    {
        const int ge = j / C, c = j - ge * C;
        const int64_t e = e0 + ge;
        const uint8_t* sl = smem_all + (size_t)(ge < EPW ? ge : 0) * g.s_total;
        const int owner = (int)reinterpret_cast<const int8_t*>(sl + g.s_rec + g.o_core_owner)[c];
        const bool v = ge < EPW && e < E && owner == 0;
        const uint32_t* crow = reinterpret_cast<const uint32_t*>(sl + g.s_scratch) + c * nw;
        const int c0 = 2 * g4, c1 = 2 * g4 + 1;
        const u4v x = bytes_to_bf16(crow[c0 < nw ? c0 : nw - 1], crow[c1 < nw ? c1 : nw - 1]);
        f4 acc[2];
        acc[0] = (f4){0, 0, 0, 0};
        acc[0] = mfma_bf16(wa.hi[0], x, acc[0]);
        acc[0] = mfma_bf16(wa.mid[0], x, acc[0]);
        acc[0] = mfma_bf16(wa.lo[0], x, acc[0]);
        acc[1] = acc[0];  // (an empty partner tile: no row of it is written)
        const int64_t item = e * C + c;
        float uu[2] = {philox_u(item), 0.f};
        int act[2];
        float lp[2];
        ha.run2(acc, A, g4, uu, act, lp);
        if (g4 == 0 && v) {
            aa.action[item] = (int8_t)act[0];
            aa.logprob[item] = lp[0];
        }
    }
    // ---- the owned cores' items: the foreign row, sampled from its table (k_act_common's scan)
    const float S = __uint_as_float(s_atab[0]);
    const int last_nz = (int)s_atab[1];
    {
        const int ge = lane / C, c = lane - ge * C;
        const int64_t e = e0 + ge;
        const uint8_t* sl = smem_all + (size_t)(ge < EPW ? ge : 0) * g.s_total;
        const bool in = lane < EPW * C && e < E;
        const int owner = (int)reinterpret_cast<const int8_t*>(sl + g.s_rec + g.o_core_owner)[c];
        if (in && owner != 0) {
            const int64_t item = e * C + c;
            const float target = philox_u(item) * S;
            int cnt = 0;
#pragma unroll
            for (int step = 16; step >= 1; step >>= 1)
                if (cnt + step <= 16 && s_acum[cnt + step - 1] <= target) cnt += step;
            const int act = cnt >= A ? last_nz : cnt;
            aa.action[item] = (int8_t)act;
            aa.logprob[item] = s_alp[act];
        }
    }
}

// fused_act and then the auctioneer's acting on the same observations
template <int LPE, class SH>
__device__ __forceinline__ void fused_act_auct(const Params& P, int64_t E, const FusedAct& fa, const AuctAct& aa,
                                               int64_t slot, int lane_arg = -1) {
    fused_act<LPE, SH>(P, E, fa, slot, lane_arg);
    auct_act<LPE, SH>(P, E, fa, aa, slot, lane_arg);
}

// ---- one round and the next round's acting of the three nets in one launch (ms_env_step_act_auct)
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 4) k_env_step_act_auct(Params P, int64_t E, uint8_t* recs, uint32_t* mt,
                                                          Liab* liab, StepIO io, FusedAct fa, AuctAct aa) {
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        io.span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    env_round<LPE, false, true, SH, MET>(P, E, recs, mt, liab, io, blockIdx.x);
    fused_act_auct<LPE, SH>(P, E, fa, aa, blockIdx.x);
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime();
        io.span[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// ---- the one-launch rollout (ms_env_rollout_act_auct): n_rounds rounds of k_env_step_act_auct, as k_env_rollout_act
//      runs k_env_step_act's (see there for the fence between rounds and the opaque argument and lane reads). Round t
//      reads its auctioneer actions from io.act_auct advanced by t strides, which for t >= 1 is what the acting after
//      round t - 1 wrote: the same lanes' stores, ordered by the fence.
struct RolloutAuctArgs {
    Params P;
    int64_t E;
    uint8_t* recs;
    uint32_t* mt;
    Liab* liab;
    StepIO io;
    FusedAct fa;
    AuctAct aa;
    AuctRollout ro;
};
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 2) k_env_rollout_act_auct(RolloutAuctArgs A0) {
    unsigned long long* span = A0.io.span;
    if (span && threadIdx.x == 0) {
        span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    const int n_rounds = A0.ro.n_rounds;
    for (int t = 0; t < n_rounds; t++) {
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();  // (see k_env_rollout_act)
        asm volatile("" : "+s"(ka));
        const RolloutAuctArgs& A = *(const RolloutAuctArgs*)ka;
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const RoundStride& st = A.ro.st;
        StepIO io = A.io;
        io.span = nullptr;
        io.act_acc = advance(io.act_acc, t * st.act_acc);
        io.act_off = advance(io.act_off, t * st.act_off);
        io.act_auct = advance(io.act_auct, t * A.ro.act_auct);
        io.obs_crow = advance(io.obs_crow, t * st.obs_crow);
        io.obs_cown = advance(io.obs_cown, t * st.obs_cown);
        io.obs_off = advance(io.obs_off, t * st.obs_off);
        io.rew_offer = advance(io.rew_offer, t * st.rew_offer);
        io.rew_acc = advance(io.rew_acc, t * st.rew_acc);
        io.rew_agent = advance(io.rew_agent, t * st.rew_agent);
        io.rew_auct = advance(io.rew_auct, t * st.rew_auct);
        env_round<LPE, false, true, SH, MET, MET>(A.P, A.E, A.recs, A.mt, A.liab, io, blockIdx.x, lane);
        if (t + 1 < n_rounds || A.ro.act_last) {
            FusedAct fa = A.fa;
            fa.off_action = advance(fa.off_action, t * st.off_action);
            fa.off_logprob = advance(fa.off_logprob, t * st.off_logprob);
            fa.acc_action = advance(fa.acc_action, t * st.acc_action);
            fa.acc_logprob = advance(fa.acc_logprob, t * st.acc_logprob);
            fa.off_offset += (uint64_t)t * st.offset_step;
            fa.acc_offset += (uint64_t)t * st.offset_step;
            AuctAct aa = A.aa;
            aa.action = advance(aa.action, t * A.ro.auct_action);
            aa.logprob = advance(aa.logprob, t * A.ro.auct_logprob);
            aa.offset += (uint64_t)t * st.offset_step;
            fused_act_auct<LPE, SH>(A.P, A.E, fa, aa, blockIdx.x, lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        wave_sync();
    }
    if (span && threadIdx.x == 0) {
        span[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime();
        span[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// ---- launch wrappers (declared in ms_env_auct_launch.h); the cases are launch_env_rollout_act's
static bool auct_launch_ok(const EnvDev& d, const StepIO& io, const AuctAct& aa) {
    return env_step_act_supported(d.P, d.E) && !d.P.free_prices && io.act_acc != nullptr && io.act_off != nullptr &&
           io.act_auct != nullptr && io.obs_acc == nullptr && aa.action != nullptr && aa.logprob != nullptr;
}
template <int LPE, class SH>
static hipError_t launch_step_act_auct_sh(const EnvDev& d, const StepIO& io, const FusedAct& fa, const AuctAct& aa,
                                          hipStream_t s) {
    constexpr int G = kWave / LPE;
    const int64_t blocks = (d.E + G - 1) / G;
    const size_t lds = (size_t)d.P.s_total * G > 4 * kMtN ? (size_t)d.P.s_total * G : 4 * kMtN;  // >= one MT block
    auto kern = io.metrics ? k_env_step_act_auct<LPE, SH, true> : k_env_step_act_auct<LPE, SH, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, d.P, d.E, d.recs, d.mt, d.liab, io, fa, aa);
    return hipGetLastError();
}
hipError_t launch_env_step_act_auct(const EnvDev& d, const StepIO& io, const FusedAct& fa, const AuctAct& aa,
                                    hipStream_t s) {
    if (!auct_launch_ok(d, io, aa)) return hipErrorInvalidValue;
    switch (lanes_per_env(d.P, d.E)) {
        case 16: return launch_step_act_auct_sh<16, DynShape>(d, io, fa, aa, s);
        case 32:
#ifndef MS_NO_FIXED_SHAPES
            if (is_shape<4, 4, 3, 1>(d.P)) return launch_step_act_auct_sh<32, FixShape<4, 4, 3, 1>>(d, io, fa, aa, s);
#endif
            return launch_step_act_auct_sh<32, DynShape>(d, io, fa, aa, s);
        default: return launch_step_act_auct_sh<64, DynShape>(d, io, fa, aa, s);
    }
}
template <int LPE, class SH>
static hipError_t launch_rollout_act_auct_sh(const RolloutAuctArgs& A, hipStream_t s) {
    constexpr int G = kWave / LPE;
    const int64_t blocks = (A.E + G - 1) / G;
    const size_t lds = (size_t)A.P.s_total * G > 4 * kMtN ? (size_t)A.P.s_total * G : 4 * kMtN;  // >= one MT block
    auto kern = A.io.metrics ? k_env_rollout_act_auct<LPE, SH, true> : k_env_rollout_act_auct<LPE, SH, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, A);
    return hipGetLastError();
}
hipError_t launch_env_rollout_act_auct(const EnvDev& d, const StepIO& io, const FusedAct& fa, const AuctAct& aa,
                                       const AuctRollout& ro, hipStream_t s) {
    if (!auct_launch_ok(d, io, aa) || io.ev_acc != nullptr || io.ev_term != nullptr || ro.n_rounds < 1)
        return hipErrorInvalidValue;
    const RolloutAuctArgs A{d.P, d.E, d.recs, d.mt, d.liab, io, fa, aa, ro};
    switch (lanes_per_env(d.P, d.E)) {
        case 16: return launch_rollout_act_auct_sh<16, DynShape>(A, s);
        case 32:
#ifndef MS_NO_FIXED_SHAPES
            if (is_shape<4, 4, 3, 1>(d.P)) return launch_rollout_act_auct_sh<32, FixShape<4, 4, 3, 1>>(A, s);
#endif
            return launch_rollout_act_auct_sh<32, DynShape>(A, s);
        default: return launch_rollout_act_auct_sh<64, DynShape>(A, s);
    }
}

}  // namespace ms

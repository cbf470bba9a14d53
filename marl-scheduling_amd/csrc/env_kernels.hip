// env_kernels.hip — the env kernels, one unit: the initial state and reset observations, one round per launch
// (k_env_step, every lane-group width and the BASELINE shapes), the auctioneer / randbelow helpers of the drop-in
// driver, the round with the next round's acting (k_env_step_act), the fixed-price one-launch rollout
// (k_env_rollout_act, BASELINE cfg2) and the free-price one (k_env_rollout_act_free with its acting act_free,
// BASELINE cfg3). The round itself and the fused acting are ms_env_round.h's; the common-item fill is a unit of its
// own (acc_fill_kernels.hip). The four families stay one unit because the compiler's choices for the round's helpers
// that are not force-inlined depend on the callers a unit holds: apart, kernels of each family compile to other
// code, and one of them ran slower (profiles/env_split/README.md).
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "ms_env_launch.h"
#include "ms_env_round.h"

namespace ms {

#ifdef MS_PHASE_TIMING
__device__ unsigned long long g_wave_span[kProbeSlots][2];    // k_env_step, last launch: s_memrealtime at entry / exit
__device__ unsigned long long g_free_cycles[kProbeSlots][5];  // k_env_rollout_act_free: env, wait, offers, acceptors, wait
// k_env_rollout_act_free, last launch, per workgroup: [0] bit 63 set, the CU rank in bit 32, the CU key below;
// [1 + k] the s_memrealtime after the round's first barrier, rounds 0..63 and the last 16 (tools/free_stagger_probe.py)
constexpr int kProbeWgs = 4096, kProbeRoundsHead = 64, kProbeRoundsTail = 16;
__device__ unsigned long long g_free_rounds[kProbeWgs][1 + kProbeRoundsHead + kProbeRoundsTail];
#endif

// ---------------------------------------------------------------------------
// kernels (the host picks LPE; init / reset / auctioneer / randbelow run one env per wave)

// Initial state (world.py:247, Core.__init__ world.py:30-37, JobCollection
// world.py:118-121) and random.seed(seed + e) (init_by_array of the seed's
// 32-bit words).
__global__ void __launch_bounds__(64) k_env_init(Params P, uint8_t* recs, uint32_t* mt, Liab* liab,
                                                 uint64_t seed) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;
    uint8_t* rec = smem;
    uint32_t* st = reinterpret_cast<uint32_t*>(smem + P.s_scratch);
    for (int i = lane; i < P.rec_bytes / 4; i += kWave) reinterpret_cast<uint32_t*>(rec)[i] = 0;
    wave_sync();
    Rec R{rec, &P, nullptr};
    for (int c = lane; c < P.C; c += kWave) {
        R.core_owner()[c] = 0;
        R.core_kind()[c] = -1;
        R.core_rem()[c] = -1;
        R.liab_n()[c] = 0;
        R.core_birth()[c] = -1;
    }
    for (int i = lane; i < P.NL; i += kWave) {
        R.slot_kind()[i] = -1;
        R.slot_rem()[i] = -1;
        R.slot_wait()[i] = 0;
        R.offer_core()[i] = -1;
        R.offer_recip()[i] = 0;
        R.offer_price()[i] = 0;
        R.slot_birth()[i] = -1;
    }
    if (lane == 0) {
        const uint64_t s = seed + (uint64_t)e;
        const uint32_t key[2] = {(uint32_t)s, (uint32_t)(s >> 32)};
        const int len = key[1] ? 2 : 1;
        st[0] = 19650218u;
        for (int i = 1; i < kMtN; i++) st[i] = 1812433253u * (st[i - 1] ^ (st[i - 1] >> 30)) + (uint32_t)i;
        int i = 1, j = 0;
        for (int k = (kMtN > len ? kMtN : len); k; k--) {
            st[i] = (st[i] ^ ((st[i - 1] ^ (st[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            i++;
            j++;
            if (i >= kMtN) {
                st[0] = st[kMtN - 1];
                i = 1;
            }
            if (j >= len) j = 0;
        }
        for (int k = kMtN - 1; k; k--) {
            st[i] = (st[i] ^ ((st[i - 1] ^ (st[i - 1] >> 30)) * 1566083941u)) - (uint32_t)i;
            i++;
            if (i >= kMtN) {
                st[0] = st[kMtN - 1];
                i = 1;
            }
        }
        st[0] = 0x80000000u;
        R.mti() = kMtN;
        R.mt_sel() = 2u;  // current = half 0, half 1 = its successor
    }
    wave_sync();
    copy_dwords<kWave>(mt + e * 2 * kMtN, st, kMtN, lane);
    wave_sync();
    mt_twist_lds_wave(st, lane);
    copy_dwords<kWave>(mt + e * 2 * kMtN + kMtN, st, kMtN, lane);
    copy_dwords<kWave>(reinterpret_cast<uint32_t*>(recs + e * (int64_t)P.rec_bytes), reinterpret_cast<uint32_t*>(rec),
                       P.rec_bytes / 4, lane);
}

__global__ void __launch_bounds__(64) k_env_reset(Params P, const uint8_t* recs, int8_t* obs_acc, int8_t* obs_off,
                                                  int8_t* obs_auct, int8_t* obs_crow, int8_t* obs_cown) {
    extern __shared__ __align__(16) uint8_t smem[];
    M128* s_mc = reinterpret_cast<M128*>(smem + P.s_mc);
    M128* s_mr = reinterpret_cast<M128*>(smem + P.s_mr);
    const int lane = threadIdx.x;
    const int64_t e = blockIdx.x;
    uint8_t* rec = smem + P.s_rec;
    __shared__ int32_t s_kt[48];
    load_kind_tables(P, s_kt, lane);
    copy_dwords<kWave>(reinterpret_cast<uint32_t*>(rec),
                       reinterpret_cast<const uint32_t*>(recs + e * (int64_t)P.rec_bytes), P.rec_bytes / 4, lane);
    wave_sync();
    Rec R{rec, &P, s_kt};
    build_masks<kWave>(R, P, s_mc, s_mr, lane);
    emit_obs<kWave>(R, P, s_mc, s_mr, smem + P.s_scratch, obs_acc, obs_off, obs_auct, obs_crow, obs_cown, e, gridDim.x,
                    true, lane);
}

// One round for the 64 / LPE envs of wave slot blockIdx.x. (A persistent loop over several slots
// per wave would let one slot's observation stores drain under the next slot's compute, but the
// compiler then keeps the whole round's state live across iterations: 3x the VGPRs.)
template <int LPE, bool EXT, bool CMP, class SH>
__global__ void __launch_bounds__(64, 4) k_env_step(Params P, int64_t E, uint8_t* recs, uint32_t* mt, Liab* liab,
                                                 StepIO io, MixIO mix) {
#ifdef MS_PHASE_TIMING
    const uint64_t rt_start = __builtin_amdgcn_s_memrealtime();
#endif
    // per-wave start / end for the bench's launch span (optional; plain stores, no shared address,
    // nothing held across the round: the kernel sits at 4 waves per SIMD with no register to spare)
    // (with the shader clock beside the 100 MHz one: the launch's effective clock, which differs box to box)
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        io.span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    env_round<LPE, EXT, CMP, SH>(P, E, recs, mt, liab, io, blockIdx.x, -1, nullptr, nullptr, EXT ? &mix : nullptr);
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime();
        io.span[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
#ifdef MS_PHASE_TIMING
    if (threadIdx.x == 0) {
        g_wave_span[blockIdx.x % kProbeSlots][0] = rt_start;
        g_wave_span[blockIdx.x % kProbeSlots][1] = __builtin_amdgcn_s_memrealtime();
    }
#endif
}

// Auctioneer.getAuctioneerAction (Auctioneer.py:95-102) on its own, as the driver calls it
// before env.step (trainPPO.py:162): writes actions [E][C] and advances the env stream by the
// tie-break draws; a following ms_env_step with these actions then draws only the spawn.
__global__ void __launch_bounds__(64) k_env_auctioneer(Params P, uint8_t* recs, uint32_t* mt, int8_t* actions) {
    extern __shared__ __align__(16) uint8_t smem[];
    M128* s_mc = reinterpret_cast<M128*>(smem + P.s_mc);
    M128* s_mr = reinterpret_cast<M128*>(smem + P.s_mr);
    int16_t* s_auct = reinterpret_cast<int16_t*>(smem + P.s_auct);
    const int lane = threadIdx.x;
    const Lanes<kWave> Lg(lane);
    const int64_t e = blockIdx.x;
    uint8_t* rec = smem + P.s_rec;
    __shared__ int32_t s_kt[48];
    mt_refill_next<kWave>(mt, recs, P, blockIdx.x, true, smem, lane);
    load_kind_tables(P, s_kt, lane);
    copy_dwords<kWave>(reinterpret_cast<uint32_t*>(rec),
                       reinterpret_cast<const uint32_t*>(recs + e * (int64_t)P.rec_bytes), P.rec_bytes / 4, lane);
    wave_sync();
    Rec R{rec, &P, s_kt};
    MtStream<kWave> rs;
    rs.init(mt + e * 2 * kMtN, R.mt_sel(), R.mti(), true);
    rs.load(0, 0, Lg);
    build_masks<kWave>(R, P, s_mc, s_mr, lane);
    hardcoded_auctioneer<kWave>(R, P, s_mc, s_mr, rs, s_auct, Lg);
    wave_sync();
    for (int c = lane; c < P.C; c += kWave) actions[e * P.C + c] = (int8_t)s_auct[c];
    if (lane == 0) {
        int32_t* hdr = reinterpret_cast<int32_t*>(recs + e * (int64_t)P.rec_bytes);
        mt_commit(rs.end_index(), hdr + 2, reinterpret_cast<uint32_t*>(hdr + 3));
    }
}

// random._randbelow(n) on env e's stream (random.randint in the update schedulers,
// Agent.py:718,725, SchedulingEnvironment.py:317-326).
__global__ void __launch_bounds__(64) k_env_randbelow(Params P, uint8_t* recs, uint32_t* mt, int64_t e, uint32_t n,
                                                      uint32_t* out) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x;
    const Lanes<kWave> Lg(lane);
    uint8_t* rec = recs + e * (int64_t)P.rec_bytes;
    int32_t* mti = reinterpret_cast<int32_t*>(rec + 8);
    uint32_t* sel = reinterpret_cast<uint32_t*>(rec + 12);
    if (!(*sel & 2u)) mt_twist_into_successor(mt + e * 2 * kMtN, *sel, smem, lane);
    MtStream<kWave> rs;
    rs.init(mt + e * 2 * kMtN, *sel, *mti, true);
    const uint32_t r = rs.randbelow(n, Lg);
    wave_sync();
    if (lane == 0) {
        *out = r;
        mt_commit(rs.end_index(), mti, sel);
    }
}

// ---- one round and the next round's acting in one launch (ms_env_step_act)
// the round of k_env_step (compact acceptor observations) and then the next round's acting (fused_act);
// MET: the round with the episode metrics (io.metrics given; env_round)
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 4) k_env_step_act(Params P, int64_t E, uint8_t* recs, uint32_t* mt, Liab* liab,
                                                     StepIO io, FusedAct fa) {
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        io.span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    env_round<LPE, false, true, SH, MET>(P, E, recs, mt, liab, io, blockIdx.x);
    fused_act<LPE, SH>(P, E, fa, blockIdx.x);
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime();
        io.span[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// k_env_step_act with a mixed population (ms_env_step_act_mixed): the agents of hc_mask play the rules in the
// round, and their rows of the round's action arrays receive the picks
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 4) k_env_step_act_mixed(Params P, int64_t E, uint8_t* recs, uint32_t* mt,
                                                           Liab* liab, StepIO io, FusedAct fa, uint64_t hc_mask) {
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        io.span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    const MixIO mix{hc_mask, nullptr, nullptr};
    env_round<LPE, false, true, SH, MET, false, true>(P, E, recs, mt, liab, io, blockIdx.x, -1, nullptr, nullptr, &mix);
    fused_act<LPE, SH>(P, E, fa, blockIdx.x);
    if (io.span && threadIdx.x == 0) {
        io.span[4 * blockIdx.x + 3] = __builtin_amdgcn_s_memtime();
        io.span[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    }
}

// ---- the fixed-price one-launch rollout (ms_env_rollout_act)
// n_rounds rounds of k_env_step_act in one launch: each wave steps its replicas, then samples their next
// actions, round after round; round t's arrays are the given ones advanced by t strides. A round reads what
// the wave's lanes wrote in the round before (records, MT blocks, liabilities, actions): a workgroup-scope
// fence (the wave is its workgroup) orders those writes before the next round's loads.
// Every round re-reads its arguments from the kernel-argument segment through a pointer the compiler cannot
// see through, and takes the lane index the same way: otherwise the loop-invariant argument loads and
// lane arithmetic are hoisted out of the round loop and held across it (hundreds of spilled registers).
struct RolloutArgs {
    Params P;
    int64_t E;
    uint8_t* recs;
    uint32_t* mt;
    Liab* liab;
    StepIO io;
    FusedAct fa;
    RoundStride st;
    int n_rounds, act_last;
};
// MET: every round adds its episode metrics (the slot follows the round's own episode; io.metrics is not strided)
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 2) k_env_rollout_act(RolloutArgs A0) {
    unsigned long long* span = A0.io.span;
    if (span && threadIdx.x == 0) {
        span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    const int n_rounds = A0.n_rounds;
    for (int t = 0; t < n_rounds; t++) {
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();  // (constant address space)
        asm volatile("" : "+s"(ka));
        const RolloutArgs& A = *(const RolloutArgs*)ka;
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const RoundStride& st = A.st;
        StepIO io = A.io;
        io.span = nullptr;
        io.act_acc = advance(io.act_acc, t * st.act_acc);
        io.act_off = advance(io.act_off, t * st.act_off);
        io.obs_crow = advance(io.obs_crow, t * st.obs_crow);
        io.obs_cown = advance(io.obs_cown, t * st.obs_cown);
        io.obs_off = advance(io.obs_off, t * st.obs_off);
        io.rew_offer = advance(io.rew_offer, t * st.rew_offer);
        io.rew_acc = advance(io.rew_acc, t * st.rew_acc);
        io.rew_agent = advance(io.rew_agent, t * st.rew_agent);
        io.rew_auct = advance(io.rew_auct, t * st.rew_auct);
        env_round<LPE, false, true, SH, MET, MET>(A.P, A.E, A.recs, A.mt, A.liab, io, blockIdx.x, lane);
        if (t + 1 < n_rounds || A.act_last) {
            FusedAct fa = A.fa;
            fa.off_action = advance(fa.off_action, t * st.off_action);
            fa.off_logprob = advance(fa.off_logprob, t * st.off_logprob);
            fa.acc_action = advance(fa.acc_action, t * st.acc_action);
            fa.acc_logprob = advance(fa.acc_logprob, t * st.acc_logprob);
            fa.off_offset += (uint64_t)t * st.offset_step;
            fa.acc_offset += (uint64_t)t * st.offset_step;
            fused_act<LPE, SH>(A.P, A.E, fa, blockIdx.x, lane);
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

// k_env_rollout_act with a mixed population (ms_env_rollout_act_mixed), the one mask for every round and replica:
// each round substitutes the masked agents' actions by the rules and writes them into its action ring slot; the
// acting samples every unit as ever, and the next round overrides the masked ones. A kernel of its own with the
// loop written out again, not a shared body: moving k_env_rollout_act's loop into a function both kernels call
// changed that kernel's register allocation and schedule (same resource figures, other code), and the plain
// rollout is to compile to exactly what it did before the mixed one existed (profiles/r14_mixed_train).
struct RolloutMixArgs {
    RolloutArgs R;
    uint64_t hc_mask;
};
template <int LPE, class SH, bool MET = false>
__global__ void __launch_bounds__(64, 2) k_env_rollout_act_mixed(RolloutMixArgs A0) {
    unsigned long long* span = A0.R.io.span;
    if (span && threadIdx.x == 0) {
        span[4 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
        span[4 * blockIdx.x + 2] = __builtin_amdgcn_s_memtime();
    }
    const int n_rounds = A0.R.n_rounds;
    for (int t = 0; t < n_rounds; t++) {
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();  // (see k_env_rollout_act)
        asm volatile("" : "+s"(ka));
        const RolloutMixArgs& M = *(const RolloutMixArgs*)ka;
        const RolloutArgs& A = M.R;
        int lane = threadIdx.x;
        asm volatile("" : "+v"(lane));
        const RoundStride& st = A.st;
        StepIO io = A.io;
        io.span = nullptr;
        io.act_acc = advance(io.act_acc, t * st.act_acc);
        io.act_off = advance(io.act_off, t * st.act_off);
        io.obs_crow = advance(io.obs_crow, t * st.obs_crow);
        io.obs_cown = advance(io.obs_cown, t * st.obs_cown);
        io.obs_off = advance(io.obs_off, t * st.obs_off);
        io.rew_offer = advance(io.rew_offer, t * st.rew_offer);
        io.rew_acc = advance(io.rew_acc, t * st.rew_acc);
        io.rew_agent = advance(io.rew_agent, t * st.rew_agent);
        io.rew_auct = advance(io.rew_auct, t * st.rew_auct);
        const MixIO mix{M.hc_mask, nullptr, nullptr};
        env_round<LPE, false, true, SH, MET, MET, true>(A.P, A.E, A.recs, A.mt, A.liab, io, blockIdx.x, lane, nullptr,
                                                        nullptr, &mix);
        if (t + 1 < n_rounds || A.act_last) {
            FusedAct fa = A.fa;
            fa.off_action = advance(fa.off_action, t * st.off_action);
            fa.off_logprob = advance(fa.off_logprob, t * st.off_logprob);
            fa.acc_action = advance(fa.acc_action, t * st.acc_action);
            fa.acc_logprob = advance(fa.acc_logprob, t * st.acc_logprob);
            fa.off_offset += (uint64_t)t * st.offset_step;
            fa.acc_offset += (uint64_t)t * st.offset_step;
            fused_act<LPE, SH>(A.P, A.E, fa, blockIdx.x, lane);
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

// ---- locally shared free-price rollouts (BASELINE cfg3; ms_env_rollout_act_free): the next round's
//      getActionForAllAgents (SchedulingEnvironment.py:150-172) of a workgroup's replicas, one wave per agent,
//      from the observations the workgroup's env round just built in its LDS: the agent's offer units
//      (FreePriceOfferPPO.selectAction PPOmodules.py:312-332: core chooser, then the price chooser on
//      [obs[2a:2a+2], obs[-2:]] or the dummy [-5] * 4) and its acceptors (LocallySharedPPO.selectAction
//      PPOmodules.py:532-543, Agent.py:682-699) on the compact acceptor rows. The arithmetic and the Philox draws
//      are k_act_pair's (act_tiles' core + price choosers with the price table, act_common_rows' compact
//      acceptors), so the outputs equal ms_act_round_free's on the emitted observations bit for bit:
//      a row's MFMA column, its four lanes' reductions and its draw depend on the row alone, not on the rows
//      that share its tile.
constexpr int kPriceTW1 = 36;  // floats per price-table entry of <= 16 actions (policy_kernels.hip PriceTW<1>)

__device__ __forceinline__ uint32_t pick4u(const uint32_t (&v)[4], int k) {
    return k == 0 ? v[0] : (k == 1 ? v[1] : (k == 2 ? v[2] : v[3]));
}

// The acceptors of cores the agent does not own are left to k_acc_common_fill (after the launch, or later on
// another stream): the env reads only the owner's acceptor action (world.py:391-404), so their sampling is off the
// round's chain. (Sampling them here as well, k_act_common's table search per item: 50.2 us per round against
// 47.4, profiles/r7g.)
// The staggered launch's acting priority (wave-uniform): the two workgroups of a CU take the upper pair of levels
// (2, 3) in turns, the other the lower pair (0, 1), by slices of 2^kFreeStaggerSlice ticks of the 100 MHz clock
// both read (rank 0 in the even slices), so neither is the older, favoured one for long. (Slices of 2^14 .. 2^18
// ticks measured alike; a fixed pair per rank and a start delay for rank 1 were slower or no different and are
// gone, profiles/r10a/ab_modes.json.)
constexpr int kFreeStaggerSlice = 16;
__device__ __forceinline__ bool stagger_upper_pair(int rank) {
    const uint32_t slice = (uint32_t)(__builtin_amdgcn_s_memrealtime() >> kFreeStaggerSlice);
    return __builtin_amdgcn_readfirstlane((int)((slice ^ (uint32_t)rank) & 1u)) == 0;
}
// SEP (the staggered kernels): prio_upper, see pace
template <class SH, int PART = 3, bool SEP = false>  // PART bit 0: the offer units, bit 1: the acceptors (the probe build times them apart)
__device__ __forceinline__ void act_free(const Geom& g, int64_t E, const FusedActFree& fa, int64_t e0, int a, int lane,
                                         uint8_t* lds, const FreeLds& fl, bool pace_on = false,
                                         int prio_upper = 0) {
    const int j = lane & 15, g4 = lane >> 4;
    // pace_on: waves a and a ^ 4 share a SIMD, where issue goes to the older wave first, so one of them finishes
    // its acting well before the other and waits at the round's barrier. After each step (a tile pair, a 64-item
    // scan) a wave counts it in the LDS and raises its issue priority while it is behind its partner.
    // prio_upper (SEP; wave-uniform: the staggered launch's priority separation): the toggle is between levels 2
    // and 3 instead of 0 and 1. (Read through an opaque copy: as a loop invariant it had the compiler build every
    // tile loop twice, 13.6k instructions for 11.9k and 200 more lane moves.)
    const int partner = a ^ 4;
    const bool pacing = pace_on && partner < g.N;
    auto pace = [&]() {
        if (!pacing) return;
        volatile int* pg = reinterpret_cast<volatile int*>(lds + fl.pace);
        const int mine = pg[a] + 1;
        pg[a] = mine;
        const int other = __builtin_amdgcn_readfirstlane(pg[partner]);
        const bool behind = other > __builtin_amdgcn_readfirstlane(mine);
        if constexpr (SEP) {
            int upper = __builtin_amdgcn_readfirstlane(prio_upper);
            asm volatile("" : "+s"(upper));
            if (upper) {
                if (behind)
                    __builtin_amdgcn_s_setprio(3);
                else
                    __builtin_amdgcn_s_setprio(2);
                return;
            }
        }
        if (behind)
            __builtin_amdgcn_s_setprio(1);
        else
            __builtin_amdgcn_s_setprio(0);
    };
    const int N = g.N, C = g.C, L = g.L, Uo = g.NL, Ua = N * C;
    const int EW = kFreeEPW * N;  // the workgroup's replicas
    const uint64_t dev_off = fa.offset_dev ? *fa.offset_dev : 0ull;
    const int16_t* pdig = reinterpret_cast<const int16_t*>(lds + fl.pdig);
    auto slice = [&](int k) -> const uint8_t* { return lds + k * g.s_total; };

    // ---------------- the offer units: agent a's L slots of every replica, rows r = k * L + s
    if constexpr ((PART & 1) != 0) {
        using FL = FragLayout<1, 1>;
        constexpr int TW = kPriceTW1;
        W1Split<1> w1;
        Head<1> h1;
        if (const uint32_t* fg = frag_groups<1, 1>(fa.core, false)) {
            const uint32_t* lf = fg + (size_t)a * FL::GB + lane * FL::LW;
            w1.load_frag(lf);
            h1.load_frag(reinterpret_cast<const float*>(lf + 12));
        } else {
            w1.load(fa.core.w1 + (size_t)a * 16 * fa.core.in_dim, fa.core.in_dim, j, g4);
            h1.load(fa.core, a, j, g4);
        }
        const int n_rows = EW * L, tiles = (n_rows + 15) >> 4;
        const uint64_t off = fa.off_offset + dev_off;
        const uint32_t rbase = (uint32_t)fa.core.row_base;
        const long long rows_all = E * Uo;
        const RawBuf ca_b(fa.core_action, rows_all), cl_b(fa.core_logprob, 4 * rows_all),
            ps_b(fa.price_state, 4 * rows_all), pa_b(fa.price_action, rows_all), pl_b(fa.price_logprob, 4 * rows_all),
            ep_b(fa.env_price, rows_all);
        const RawBuf tab_b(fa.ptab + (size_t)a * fa.pkeys * TW, 4ll * fa.pkeys * TW);
        const int nwo = g.off_stride >> 2, pcol = (2 * C) >> 2, pshift = 8 * ((2 * C) & 3);
        const int A1 = fa.core.n_actions, A2 = fa.price.n_actions;
        // the call row (e * N*L + a*L + s) of the agent's row r, -1 past the replicas; k, s: its replica in
        // the workgroup and its slot (0 for rows past the end: their LDS reads stay in range)
        auto row_of = [&](int r, int& k, int& s) -> int {
            k = r / L;
            s = r - k * L;
            const bool v = r < n_rows && e0 + k < E;
            const int row = (int)((e0 + k) * Uo) + a * L + s;
            if (r >= n_rows) k = s = 0;
            return v ? row : -1;
        };
        uint32_t rb0[4] = {0, 0, 0, 0}, rb1[4] = {0, 0, 0, 0};
        // one tile pair up to the price chooser's input: the rows' core choices, the price inputs and their
        // key digits (act_tiles: core2 + price_in2)
        auto core_pair = [&](int tile, int (&cur)[2], int (&act)[2], float (&lp)[2], float (&u2)[2], int (&pin)[2],
                             int (&dg)[2]) {
            if ((tile & 3) == 0) {  // Philox for 4 tiles: lane (j, g4) draws row j of tile tile + g4
                int k, s;
                const int r = row_of(16 * (tile + g4) + j, k, s);
                uint32_t r0, r1;
                philox2((uint32_t)r + rbase, off, fa.seed, r0, r1);
                rows_bcast(r1, rb1);
                rows_bcast(r0, rb0);
            }
            const int kq = tile & 3;
            int kk[2], ss[2];
            f4 acc[2];
            float u1[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                cur[i] = row_of(16 * (tile + i) + j, kk[i], ss[i]);
                const uint8_t* sc = slice(kk[i]) + g.s_scratch;
                const uint32_t* otmpl = reinterpret_cast<const uint32_t*>(sc + g.s_otmpl);
                const uint32_t pr = reinterpret_cast<const uint16_t*>(sc + g.s_slotpair)[a * L + ss[i]];
                uint32_t d[2];
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const int cc = 2 * g4 + h, wd = cc < nwo ? cc : nwo - 1;
                    d[h] = otmpl[wd] | (wd == pcol ? pr << pshift : 0u);
                }
                const u4v x = bytes_to_bf16(d[0], d[1]);
                acc[i] = (f4){0, 0, 0, 0};
                acc[i] = mfma_bf16(w1.hi[0], x, acc[i]);
                acc[i] = mfma_bf16(w1.mid[0], x, acc[i]);
                acc[i] = mfma_bf16(w1.lo[0], x, acc[i]);
                u1[i] = u24(pick4u(rb0, kq + i));
                u2[i] = u24(pick4u(rb1, kq + i));
            }
            h1.run2(acc, A1, g4, u1, act, lp);
#pragma unroll
            for (int i = 0; i < 2; i++) {
                // byte kb of the row: the chosen core's (prio, rem) for g4 < 2, the slot's pair obs[-2:] for g4 >= 2
                const int kb = g4 < 2 ? 2 * act[i] + g4 : 2 * C + (g4 - 2);
                const int8_t* sc = reinterpret_cast<const int8_t*>(slice(kk[i]) + g.s_scratch);
                const int byte = kb < 2 * C ? sc[g.s_otmpl + kb] : sc[g.s_slotpair + 2 * (a * L + ss[i]) + (kb - 2 * C)];
                pin[i] = act[i] == 0 ? -5 : byte;
                dg[i] = cur[i] >= 0 ? (int)pdig[g4 * 256 + pin[i] + 128] : 0;
            }
        };
        // the price chooser's outputs of a pair (PPOmodules.py:316-332; env price -5 for core action 0)
        auto price_out = [&](const int (&cur)[2], const int (&act)[2], const int (&pin)[2], const int (&pact)[2],
                             const float (&plp)[2]) {
#pragma unroll
            for (int i = 0; i < 2; i++)
                if (cur[i] >= 0) {
                    const uint32_t pc = (uint32_t)cur[i];
                    ps_b.st8(4 * pc + g4, pin[i]);
                    if (g4 == 0) {
                        pa_b.st8(pc, pact[i]);
                        pl_b.stf(4 * pc, plp[i]);
                        ep_b.st8(pc, act[i] == 0 ? -5 : pact[i]);
                    }
                }
        };
        bool any_miss = false;
        for (int tile = 0; tile < tiles; tile += 2) {
            int cur[2], act[2], pin[2], dg[2];
            float lp[2], u2[2];
            core_pair(tile, cur, act, lp, u2, pin, dg);
            if (__ballot(dg[0] < 0 || dg[1] < 0) == 0ull) {
                // every row of the pair is tabulated: sample from the table (act_tiles' arithmetic)
                rows_sum2_i(dg[0], dg[1]);
                float cum[2][4], S2[2];
                int lnz[2], cnt[2], pact[2];
                float plp[2];
                uint32_t te[2];
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    te[i] = __umul24((uint32_t)dg[i], 4u * TW);
                    const auto c4 = __builtin_amdgcn_raw_buffer_load_b128(tab_b.r, (int)(te[i] + 4 * (4 * g4)), 0, 0);
#pragma unroll
                    for (int q = 0; q < 4; q++) cum[i][q] = __uint_as_float(c4[q]);
                    S2[i] = tab_b.ldf(te[i] + 4 * 32);
                    lnz[i] = (int)tab_b.ld32(te[i] + 4 * 33);
                }
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    const float target = u2[i] * S2[i];
                    cnt[i] = 0;
#pragma unroll
                    for (int q = 0; q < 4; q++) cnt[i] += (cum[i][q] <= target) ? 1 : 0;
                }
                rows_sum2_i(cnt[0], cnt[1]);
#pragma unroll
                for (int i = 0; i < 2; i++) {
                    pact[i] = cnt[i] >= A2 ? lnz[i] : cnt[i];
                    plp[i] = tab_b.ldf(te[i] + 4 * (16 + pact[i]));
                }
                price_out(cur, act, pin, pact, plp);
            } else {
                any_miss = true;
            }
#pragma unroll
            for (int i = 0; i < 2; i++)
                if (cur[i] >= 0 && g4 == 0) {
                    ca_b.st8((uint32_t)cur[i], act[i]);
                    cl_b.stf(4 * (uint32_t)cur[i], lp[i]);
                }
            pace();
        }
        if (any_miss) {
            // the pairs the table could not serve: the same pairs and draws again, the core chooser recomputed
            // (bit-identical), then the price net itself (act_tiles' second loop)
            Head<1> h2;
            h2.load(fa.price, a, j, g4);
            const float pw1 = fa.price.w1[((size_t)a * 16 + j) * 4 + g4];  // W1p[j][g4] (K = 4 inputs)
            for (int tile = 0; tile < tiles; tile += 2) {
                int cur[2], act[2], pin[2], dg[2];
                float lp[2], u2[2];
                core_pair(tile, cur, act, lp, u2, pin, dg);
                if (__ballot(dg[0] < 0 || dg[1] < 0) == 0ull) continue;  // priced from the table above
                int pact[2];
                float plp[2];
                f4 acc2[2];
#pragma unroll
                for (int i = 0; i < 2; i++) acc2[i] = mfma4(pw1, (float)pin[i], (f4){0, 0, 0, 0});
                h2.run2(acc2, A2, g4, u2, pact, plp);
                price_out(cur, act, pin, pact, plp);
            }
        }
    }

    // ---------------- the acceptors: agent a's C items of every replica, item m = k * C + c (group item
    //                  i = e * C + c): the cores it does not own sample the common row's table, the owned ones
    //                  are listed and run in 16-row MFMA tiles (act_common_rows with compact rows)
    if constexpr ((PART & 2) != 0) {
        using FL = FragLayout<2, 2>;
        const uint32_t* const fg = frag_groups<2, 2>(fa.acc, true);
        int16_t* lm = reinterpret_cast<int16_t*>(lds + fl.list + a * kFreeListCap * 6);
        float* lu = reinterpret_cast<float*>(lds + fl.list + a * kFreeListCap * 6 + 2 * kFreeListCap);
        const int nw = g.acc_stride >> 2, Aa = fa.acc.n_actions;
        const int n_items = EW * C;
        const uint64_t off = fa.acc_offset + dev_off;
        const uint32_t rbase = (uint32_t)fa.acc.row_base;
        const long long rows_all = E * Ua;
        const RawBuf aa_b(fa.acc_action, rows_all), al_b(fa.acc_logprob, 4 * rows_all);
        const RawBuf oa_b(fa.own_action, E * C), ol_b(fa.own_logprob, 4 * E * C);
        // the listed rows [0, cnt) (cnt <= 32) as two 16-row tiles (a lone or partial tile: rows past cnt
        // are computed on entry 0 and not written)
        auto tiles2 = [&](int cnt) {
            // the net's fragments only for the tiles (52 registers not held through the scan): loaded per call
            // through a pointer the compiler cannot see through, so the loads are not hoisted out of the scan loop
            W1Split<2> w1;
            Head<2> h1;
            if (fg) {
                const uint32_t* lf = fg + (size_t)a * FL::GB + lane * FL::LW;
                asm volatile("" : "+v"(lf));
                w1.load_frag(lf);
                h1.load_frag(reinterpret_cast<const float*>(lf + 24));
            } else {
                w1.load(fa.acc.w1 + (size_t)a * 16 * fa.acc.in_dim, fa.acc.in_dim, j, g4);
                h1.load(fa.acc, a, j, g4);
            }
            f4 acc[2];
            int row[2], orow[2], lrow[2];
            float uu[2];
#pragma unroll
            for (int i = 0; i < 2; i++) {
                const int t = 16 * i + j;
                const bool v = t < cnt;
                const int mm = lm[v ? t : 0];
                uu[i] = lu[v ? t : 0];
                const int kk = mm / C, cc = mm - kk * C;
                row[i] = v ? (int)((e0 + kk) * Ua) + a * C + cc : -1;
                orow[i] = (int)(e0 * C) + mm;  // (e0 + kk) * C + cc
                lrow[i] = fl.accx + kk * Ua + a * C + cc;
                const uint32_t* crow = reinterpret_cast<const uint32_t*>(slice(kk) + g.s_scratch) + cc * nw;
                acc[i] = (f4){0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const int c0 = 8 * s + 2 * g4, c1 = c0 + 1;
                    const u4v x = bytes_to_bf16(crow[c0 < nw ? c0 : nw - 1], crow[c1 < nw ? c1 : nw - 1]);
                    acc[i] = mfma_bf16(w1.hi[s], x, acc[i]);
                    acc[i] = mfma_bf16(w1.mid[s], x, acc[i]);
                    acc[i] = mfma_bf16(w1.lo[s], x, acc[i]);
                }
            }
            int act[2];
            float lp[2];
            h1.run2(acc, Aa, g4, uu, act, lp);
#pragma unroll
            for (int i = 0; i < 2; i++)
                if (row[i] >= 0 && g4 == 0) {
                    if (fa.own_action) {
                        // by core (the fill writes the rings' rows whole), and into the replica's LDS staging of
                        // acceptor actions, where the next env round reads its owners' (StepIO::acc_in_lds)
                        oa_b.st8((uint32_t)orow[i], act[i]);
                        ol_b.stf(4 * (uint32_t)orow[i], lp[i]);
                        reinterpret_cast<int8_t*>(lds)[lrow[i]] = (int8_t)act[i];
                    } else {
                        aa_b.st8((uint32_t)row[i], act[i]);
                        al_b.stf(4 * (uint32_t)row[i], lp[i]);
                    }
                }
        };
        // item i's uniform: word (i >> 6) & 1 of the draw countered by the row of item i & ~64 (k_act_common's
        // rule), so a lane's draw serves its item and the item 64 further when both are in this wave
        const uint32_t i_base = (uint32_t)(e0 * C);
        uint32_t last_ib = 0xffffffffu, wd0 = 0, wd1 = 0;
        const uint64_t below = (1ull << lane) - 1ull;
        int n_list = 0;
        for (int m0 = 0; m0 < n_items; m0 += 64) {
            const int m = m0 + lane;
            const bool in = m < n_items;
            const int k = in ? m / C : 0, c = in ? m - (m / C) * C : 0;
            const bool valid = in && e0 + k < E;
            const uint32_t i = i_base + (uint32_t)m, ib = i & ~64u;
            const int own = reinterpret_cast<const int8_t*>(slice(k) + g.s_rec + g.o_core_owner)[c];
            const bool owned = valid && own == a + 1;
            // (only the owned items' uniforms: the common ones are sampled after the launch)
            const bool need = owned && ib != last_ib;
            if (__ballot(need)) {
                const uint32_t eb = ib / (uint32_t)C;
                uint32_t r0, r1;
                philox2(eb * (uint32_t)Ua + (uint32_t)(a * C) + (ib - eb * (uint32_t)C) + rbase, off, fa.seed, r0, r1);
                if (need) {
                    last_ib = ib;
                    wd0 = r0;
                    wd1 = r1;
                }
            }
            const float u = u24((i & 64u) ? wd1 : wd0);
            const uint64_t mo = __ballot(owned);
            if (owned) {
                const int p = n_list + __popcll(mo & below);
                lm[p] = (int16_t)m;
                lu[p] = u;
            }
            n_list += __popcll(mo);
            pace();
            wave_sync();
            while (n_list >= 32) {
                tiles2(32);
                const int rest = n_list - 32;  // < 64: carried to the front of the list
                int16_t vm = 0;
                float vu = 0.f;
                if (lane < rest) {
                    vm = lm[32 + lane];
                    vu = lu[32 + lane];
                }
                wave_sync();
                if (lane < rest) {
                    lm[lane] = vm;
                    lu[lane] = vu;
                }
                wave_sync();
                n_list = rest;
            }
        }
        if (n_list > 0) tiles2(n_list);
    }
}

struct RolloutFreeArgs {
    Params P;
    int64_t E;
    uint8_t* recs;
    uint32_t* mt;
    Liab* liab;
    StepIO io;
    FusedActFree fa;
    RoundStrideFree st;
    int n_rounds, act_last;
    // The launcher's constants kFreePrio and kFreeSeparate. They are arguments, and the branches they select stay
    // in the kernel, because the kernel without them came out slower (profiles/r11_knobs).
    int prio;      // bit 0: the workgroup's waves 4.. at raised issue priority while acting, bit 1: during the env
                   // round, bit 2: the acting's waves paced against their SIMD partners (act_free pace_on)
    int separate;  // (STAG kernels) != 0: the env rounds at priority 3, the acting by stagger_upper_pair
    OffCompact oc;  // tmpl set: the rounds' offer observations compact, the rows by the last round alone
};
// The CU a wave runs on, 12 bits: HW_REG_XCC_ID's XCC above HW_REG_HW_ID's SE, SH and CU fields (bits 15..8).
constexpr int kCuKeys = 1 << 12;
__device__ __forceinline__ uint32_t cu_key() {
    const uint32_t cu = __builtin_amdgcn_s_getreg(4 | (8 << 6) | (7 << 11));  // HW_ID, offset 8, 8 bits
    const uint32_t xcc = __builtin_amdgcn_s_getreg(20 | (3 << 11));          // XCC_ID, offset 0, 4 bits
    return (xcc << 8 | cu) & (kCuKeys - 1);
}
// Arrivals per CU of the staggered launches' workgroups, never reset: a CU that holds two workgroups of a launch
// gets two arrivals per launch, so the parity of a ticket tells them apart in every launch. Only the timing of a
// workgroup depends on its ticket; nothing waits for another workgroup's.
__device__ uint32_t g_cu_ticket[kCuKeys];
// The locally shared free-price rollout in one launch: workgroup b holds replicas kFreeEPW * N * b .. in its LDS,
// and wave w steps kFreeEPW of them (k_env_step's round, 16 lanes per replica) and then acts for agent w of all
// of them (act_free), round after round, with a workgroup barrier between the phases: every agent's nets
// act from registers and LDS on the rows the round just built, instead of an act launch re-reading them from
// HBM. Round t's arrays are the given ones advanced by t strides. The round re-reads its arguments through
// the opaque kernel-argument pointer (k_env_rollout_act). Two workgroups per CU: 4 waves per SIMD (<= 128 VGPRs).
// MET: every round adds its episode metrics (env_round; the padding groups of a partial last workgroup add nothing).
// STAG (MS_FREE_STAGGER != 0): the two workgroups of a CU told apart. Left alone they drift to a random phase
// within a few rounds, and the older one, which wins issue, runs its rounds a quarter faster and leaves the other
// to finish alone (profiles/r10a). Each workgroup takes a rank from its CU's ticket (g_cu_ticket): the env phase
// runs at the highest priority and the two ranks take the higher acting priority in turns (stagger_upper_pair).
// A workgroup's results do not depend on its rank.
template <class SH, bool MET = false, bool STAG = false>
__global__ void __launch_bounds__(512, 4) k_env_rollout_act_free(RolloutFreeArgs A0) {
    extern __shared__ __align__(16) uint8_t smem_free[];
    Geom g;
    if constexpr (SH::kStatic) {
        constexpr Geom kg = make_geom(SH::kN, SH::kC, SH::kL, SH::kJ);
        g = kg;
    } else {
        g = A0.P;
    }
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int lane0 = (int)threadIdx.x & 63;
    const FreeLds fl = free_lds(g);
    const int64_t wslot = (int64_t)blockIdx.x * g.N + wave;  // the wave's slot of kFreeEPW replicas
    unsigned long long* span = A0.io.span;
    if (span && lane0 == 0) {
        span[4 * wslot] = __builtin_amdgcn_s_memrealtime();
        span[4 * wslot + 2] = __builtin_amdgcn_s_memtime();
    }
    // once per launch (the acting nets do not change within a rollout): the price table's key digits, one copy
    // per workgroup
    {
        uint32_t* pd = reinterpret_cast<uint32_t*>(smem_free + fl.pdig);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(A0.fa.pdigit);
        for (int k = (int)threadIdx.x; k < 512; k += (int)blockDim.x) pd[k] = src[k];
        // (by-core mode) the acceptor actions the env rounds stage from the LDS: the acting writes the owners'
        // items only, and the env checks every item's range (k_env_step: they are all sampled), so the others
        // hold a valid action (0, "reject") instead of whatever the LDS held
        uint32_t* ax = reinterpret_cast<uint32_t*>(smem_free + fl.accx);
        for (int k = (int)threadIdx.x; k < (fl.total - fl.accx) / 4; k += (int)blockDim.x) ax[k] = 0u;  // (+ pace)
    }
    __syncthreads();
    [[maybe_unused]] int prio_rank = -1;  // < 0: no separation
    [[maybe_unused]] int rank = 0;
    if constexpr (STAG) {
        // the rank goes through wave 0's pace word, which is free until the first acting: written back to zero
        // after every wave has read it, and the round's first barrier comes before any wave paces
        volatile int* pg = reinterpret_cast<volatile int*>(smem_free + fl.pace);
        if (threadIdx.x == 0) pg[0] = (int)(atomicAdd(&g_cu_ticket[cu_key()], 1u) & 1u);
        __syncthreads();
        rank = __builtin_amdgcn_readfirstlane(pg[0]);
        __syncthreads();
        if (threadIdx.x == 0) pg[0] = 0;
        if (A0.separate) prio_rank = rank;
    }
#ifdef MS_PHASE_TIMING
    if (threadIdx.x == 0 && blockIdx.x < kProbeWgs)
        g_free_rounds[blockIdx.x][0] = 1ull << 63 | (unsigned long long)rank << 32 | cu_key();
    // probe build: per wave, the shader cycles of the env rounds, the wait at the barrier after them, the acting,
    // and the wait at the barrier after it (tools/env_phase_probe.py --free)
    uint64_t f_prev = __builtin_amdgcn_s_memtime(), f_acc[5] = {0, 0, 0, 0, 0};
#define FREE_MARK(k)                                                   \
    do {                                                               \
        const uint64_t f_now = __builtin_amdgcn_s_memtime();          \
        if ((k) >= 0) f_acc[(k) < 0 ? 0 : (k)] += f_now - f_prev;      \
        f_prev = f_now;                                                \
    } while (0)
#else
#define FREE_MARK(k) \
    do {             \
    } while (0)
#endif
    const int n_rounds = A0.n_rounds;
    for (int t = 0; t < n_rounds; t++) {
        auto ka = __builtin_amdgcn_kernarg_segment_ptr();  // (constant address space)
        asm volatile("" : "+s"(ka));
        const RolloutFreeArgs& A = *(const RolloutFreeArgs*)ka;
        int lane = (int)threadIdx.x & 63;
        asm volatile("" : "+v"(lane));
        const RoundStrideFree& st = A.st;
        StepIO io = A.io;
        io.span = nullptr;
        io.act_acc = advance(io.act_acc, t * st.act_acc);
        io.act_off = advance(io.act_off, t * st.act_off);
        io.obs_crow = advance(io.obs_crow, t * st.obs_crow);
        io.obs_cown = advance(io.obs_cown, t * st.obs_cown);
        io.obs_off = advance(io.obs_off, t * st.obs_off);
        io.rew_offer = advance(io.rew_offer, t * st.rew_offer);
        io.rew_price = advance(io.rew_price, t * st.rew_price);
        io.rew_acc = advance(io.rew_acc, t * st.rew_acc);
        io.rew_agent = advance(io.rew_agent, t * st.rew_agent);
        io.rew_auct = advance(io.rew_auct, t * st.rew_auct);
        // compact offer observations: the template and the pairs every round; the acting below reads the LDS
        // sources either way, and the rows are for whoever reads the launch's last observation
        int8_t* const oc_tmpl = advance(A.oc.tmpl, t * A.oc.tmpl_stride);
        uint16_t* const oc_pair = advance(A.oc.pair, t * A.oc.pair_stride);
        if (oc_tmpl && t + 1 < n_rounds) io.obs_off = nullptr;
        FREE_MARK(-1);
        // (the younger half of the workgroup's waves otherwise trails the older at every barrier: issue goes by
        //  priority, then age)
        const bool up = wave >= 4 && (A.prio & 2);
        if (up) __builtin_amdgcn_s_setprio(1);
        [[maybe_unused]] int prio_upper = 0;
        if constexpr (STAG) {
            prio_rank = __builtin_amdgcn_readfirstlane(prio_rank);
            asm volatile("" : "+s"(prio_rank));  // (not a loop invariant to the compiler, as in act_free's pace)
            if (prio_rank >= 0) __builtin_amdgcn_s_setprio(3);
        }
        // rounds after the first (by-core mode): the owners' acceptor actions are where this launch's acting left
        // them in the LDS (the rings' acceptor rows are written after the launch, by the fill)
        const int8_t* acc_lds = t > 0 && A.fa.own_action
                                    ? reinterpret_cast<const int8_t*>(smem_free + fl.accx) + wave * kFreeEPW * g.N * g.C
                                    : nullptr;
        env_round<kWave / kFreeEPW, false, true, SH, MET, MET, false, true>(
            A.P, A.E, A.recs, A.mt, A.liab, io, wslot, lane, smem_free + wave * free_slot(g), acc_lds, nullptr, oc_tmpl,
            oc_pair);
        if (up) __builtin_amdgcn_s_setprio(0);
        if constexpr (STAG) {
            if (prio_rank >= 0) {  // this round's acting: the pair by now's clock slice
                prio_upper = stagger_upper_pair(prio_rank) ? 1 : 0;
                if (prio_upper)
                    __builtin_amdgcn_s_setprio(2);
                else
                    __builtin_amdgcn_s_setprio(0);
            }
        }
        FREE_MARK(0);
        if (t + 1 < n_rounds || A.act_last) {
            __syncthreads();  // every replica's observation sources are in the LDS
            FREE_MARK(1);
#ifdef MS_PHASE_TIMING
            if (threadIdx.x == 0 && blockIdx.x < kProbeWgs) {
                const int tail = t - (n_rounds - kProbeRoundsTail);
                const int k = t < kProbeRoundsHead ? t : (tail >= 0 ? kProbeRoundsHead + tail : -1);
                if (k >= 0) g_free_rounds[blockIdx.x][1 + k] = __builtin_amdgcn_s_memrealtime();
            }
#endif
            FusedActFree fa = A.fa;
            fa.core_action = advance(fa.core_action, t * st.core_action);
            fa.core_logprob = advance(fa.core_logprob, t * st.core_logprob);
            fa.price_state = advance(fa.price_state, t * st.price_state);
            fa.price_action = advance(fa.price_action, t * st.price_action);
            fa.price_logprob = advance(fa.price_logprob, t * st.price_logprob);
            fa.acc_action = advance(fa.acc_action, t * st.acc_action);
            fa.acc_logprob = advance(fa.acc_logprob, t * st.acc_logprob);
            fa.own_action = advance(fa.own_action, t * st.own_action);
            fa.own_logprob = advance(fa.own_logprob, t * st.own_logprob);
            fa.off_offset += (uint64_t)t * st.offset_step;
            fa.acc_offset += (uint64_t)t * st.offset_step;
            const bool up_act = wave >= 4 && (A.prio & 1);
            if (up_act) __builtin_amdgcn_s_setprio(1);
            const bool pace_on = (A.prio & 4) != 0;
#ifdef MS_PHASE_TIMING
            act_free<SH, 1, STAG>(g, A.E, fa, (int64_t)blockIdx.x * kFreeEPW * g.N, wave, lane, smem_free, fl, pace_on, prio_upper);
            FREE_MARK(2);
            act_free<SH, 2, STAG>(g, A.E, fa, (int64_t)blockIdx.x * kFreeEPW * g.N, wave, lane, smem_free, fl, pace_on, prio_upper);
#else
            act_free<SH, 3, STAG>(g, A.E, fa, (int64_t)blockIdx.x * kFreeEPW * g.N, wave, lane, smem_free, fl, pace_on, prio_upper);
#endif
            if (up_act || pace_on) __builtin_amdgcn_s_setprio(0);
            FREE_MARK(3);
            __syncthreads();  // the actions are stored and the LDS is free for the next round
            FREE_MARK(4);
        }
    }
    if (span && lane0 == 0) {
        span[4 * wslot + 3] = __builtin_amdgcn_s_memtime();
        span[4 * wslot + 1] = __builtin_amdgcn_s_memrealtime();
    }
#ifdef MS_PHASE_TIMING
    if (lane0 == 0)
        for (int k = 0; k < 5; k++) g_free_cycles[wslot % kProbeSlots][k] += f_acc[k];
#endif
}

}  // namespace ms

// Diagnostic, not part of the ABI (tests, tools): the tickets the staggered rollout launches have taken so far on
// the current device, one per workgroup (synchronises the device).
extern "C" long long ms_free_stagger_tickets(void) {
    static uint32_t host[ms::kCuKeys];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_cu_ticket), sizeof(host)) != hipSuccess) return -1;
    long long n = 0;
    for (int k = 0; k < ms::kCuKeys; k++) n += host[k];
    return n;
}

#ifdef MS_PHASE_TIMING
// profiling build only: read (and optionally clear) the per-phase cycle counters
extern "C" int ms_probe_phase_cycles(unsigned long long* out, int clear) {
    static unsigned long long host[ms::kProbeSlots][16];
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_phase_cycles), sizeof(host)) != hipSuccess) return -1;
    for (int k = 0; k < 16; k++) {
        out[k] = 0;
        for (int b = 0; b < ms::kProbeSlots; b++) out[k] += host[b][k];
    }
    if (clear) {
        memset(host, 0, sizeof(host));
        if (hipMemcpyToSymbol(HIP_SYMBOL(ms::g_phase_cycles), host, sizeof(host)) != hipSuccess) return -1;
    }
    return 0;
}
// the per-phase cycles of every block (summed over the launches since the last clear): out[16 * n_blocks]
extern "C" int ms_probe_phase_blocks(unsigned long long* out, int n_blocks) {
    static unsigned long long host[ms::kProbeSlots][16];
    if (n_blocks > ms::kProbeSlots) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_phase_cycles), sizeof(host)) != hipSuccess) return -1;
    memcpy(out, host, sizeof(unsigned long long) * 16 * n_blocks);
    return 0;
}
// k_env_rollout_act_free's per-wave cycles (env rounds, barrier wait, acting, barrier wait) summed over the
// launches since the last clear: out[4 * n_waves]
extern "C" int ms_probe_free_cycles(unsigned long long* out, int n_waves, int clear) {
    static unsigned long long host[ms::kProbeSlots][5];
    if (n_waves > ms::kProbeSlots) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_free_cycles), sizeof(host)) != hipSuccess) return -1;
    memcpy(out, host, sizeof(unsigned long long) * 5 * n_waves);
    if (clear) {
        memset(host, 0, sizeof(host));
        if (hipMemcpyToSymbol(HIP_SYMBOL(ms::g_free_cycles), host, sizeof(host)) != hipSuccess) return -1;
    }
    return 0;
}
// entry / exit s_memrealtime (100 MHz) of every block of the last launch: out[2 * n_blocks]
extern "C" int ms_probe_wave_spans(unsigned long long* out, int n_blocks) {
    static unsigned long long host[ms::kProbeSlots][2];
    if (n_blocks > ms::kProbeSlots) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_wave_span), sizeof(host)) != hipSuccess) return -1;
    memcpy(out, host, sizeof(unsigned long long) * 2 * n_blocks);
    return 0;
}
// k_env_rollout_act_free's last launch: out[81 * n_wgs], per workgroup its CU word and round stamps (g_free_rounds)
extern "C" int ms_probe_free_rounds(unsigned long long* out, int n_wgs) {
    constexpr int W = 1 + ms::kProbeRoundsHead + ms::kProbeRoundsTail;
    static unsigned long long host[ms::kProbeWgs][W];
    if (n_wgs > ms::kProbeWgs) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(ms::g_free_rounds), sizeof(host)) != hipSuccess) return -1;
    memcpy(out, host, sizeof(unsigned long long) * W * n_wgs);
    return 0;
}
#endif

// launch wrappers used by capi.cpp (declared in ms_env_launch.h); the kernels take an EnvDev's fields one by one
namespace ms {
hipError_t launch_env_init(const EnvDev& d, uint64_t seed, hipStream_t s) {
    const Params& P = d.P;
    // the seeding runs in the scratch, which k_env_init needs at MT-state size
    const size_t lds = (size_t)P.s_scratch + 4 * kMtN > (size_t)P.s_total ? (size_t)P.s_scratch + 4 * kMtN : P.s_total;
    hipLaunchKernelGGL(k_env_init, dim3((unsigned)d.E), dim3(kWave), lds, s, P, d.recs, d.mt, d.liab, seed);
    return hipGetLastError();
}
hipError_t launch_env_reset(const EnvDev& d, const StepIO& io, hipStream_t s) {
    hipLaunchKernelGGL(k_env_reset, dim3((unsigned)d.E), dim3(kWave), d.P.s_total, s, d.P, d.recs, io.obs_acc,
                       io.obs_off, io.obs_auct, io.obs_crow, io.obs_cown);
    return hipGetLastError();
}

template <int LPE, class SH>
static hipError_t launch_step_sh(const EnvDev& d, const StepIO& io, const MixIO& mix, hipStream_t s) {
    constexpr int G = kWave / LPE;
    const int64_t blocks = (d.E + G - 1) / G;
    const size_t lds = (size_t)d.P.s_total * G > 4 * kMtN ? (size_t)d.P.s_total * G : 4 * kMtN;  // >= one MT block
    const bool compact = io.obs_crow != nullptr || io.obs_cown != nullptr;
    // a mixed round (a mask, or the taken actions asked for) runs in the kernel of the optional features
    const bool mixed = mix.hc_mask != 0 || mix.acc_taken != nullptr || mix.off_taken != nullptr;
    const bool ext = io.act_acc == nullptr || io.metrics != nullptr || (compact && io.obs_acc != nullptr) || mixed;
    auto kern = ext ? k_env_step<LPE, true, false, DynShape>
                    : (compact ? k_env_step<LPE, false, true, SH> : k_env_step<LPE, false, false, SH>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, d.P, d.E, d.recs, d.mt, d.liab, io, mix);
    return hipGetLastError();
}

// The BASELINE shapes (cfg2 4x4x3, cfg3 8x8x3, cfg4 16x16x3, cfg5 32x32x3, one new job per agent and
// round) run the kernel compiled for their geometry; every other shape the generic one.
template <int LPE>
static hipError_t launch_step_t(const EnvDev& d, const StepIO& io, const MixIO& mix, hipStream_t s) {
#ifndef MS_NO_FIXED_SHAPES
    if constexpr (LPE == 16) {
        if (is_shape<8, 8, 3, 1>(d.P)) return launch_step_sh<LPE, FixShape<8, 8, 3, 1>>(d, io, mix, s);
        if (is_shape<16, 16, 3, 1>(d.P)) return launch_step_sh<LPE, FixShape<16, 16, 3, 1>>(d, io, mix, s);
    }
    if constexpr (LPE == 32) {
        if (is_shape<4, 4, 3, 1>(d.P)) return launch_step_sh<LPE, FixShape<4, 4, 3, 1>>(d, io, mix, s);
        if (is_shape<32, 32, 3, 1>(d.P)) return launch_step_sh<LPE, FixShape<32, 32, 3, 1>>(d, io, mix, s);
    }
#endif
    return launch_step_sh<LPE, DynShape>(d, io, mix, s);
}

hipError_t launch_env_step(const EnvDev& d, const StepIO& io, const MixIO& mix, hipStream_t s) {
    switch (lanes_per_env(d.P, d.E)) {
#if MS_MIN_LPE <= 8
        case 8: return launch_step_t<8>(d, io, mix, s);
#endif
        case 16: return launch_step_t<16>(d, io, mix, s);
        case 32: return launch_step_t<32>(d, io, mix, s);
        default: return launch_step_t<64>(d, io, mix, s);
    }
}
hipError_t launch_env_auctioneer(const EnvDev& d, int8_t* actions, hipStream_t s) {
    const size_t lds = (size_t)d.P.s_total > 4 * kMtN ? (size_t)d.P.s_total : 4 * kMtN;
    hipLaunchKernelGGL(k_env_auctioneer, dim3((unsigned)d.E), dim3(kWave), lds, s, d.P, d.recs, d.mt, actions);
    return hipGetLastError();
}
hipError_t launch_env_randbelow(const EnvDev& d, int64_t e, uint32_t n, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_env_randbelow, dim3(1), dim3(kWave), 4 * kMtN, s, d.P, d.recs, d.mt, e, n, out);
    return hipGetLastError();
}
template <int LPE, class SH>
static hipError_t launch_step_act_sh(const EnvDev& d, const StepIO& io, const FusedAct& fa, uint64_t hc_mask,
                                     hipStream_t s) {
    constexpr int G = kWave / LPE;
    const int64_t blocks = (d.E + G - 1) / G;
    const size_t lds = (size_t)d.P.s_total * G > 4 * kMtN ? (size_t)d.P.s_total * G : 4 * kMtN;  // >= one MT block
    if (hc_mask) {  // a mixed population (ms_env_step_act_mixed); no mask: the plain kernels
        auto kern = io.metrics ? k_env_step_act_mixed<LPE, SH, true> : k_env_step_act_mixed<LPE, SH, false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, d.P, d.E, d.recs, d.mt, d.liab, io, fa,
                           hc_mask);
        return hipGetLastError();
    }
    auto kern = io.metrics ? k_env_step_act<LPE, SH, true> : k_env_step_act<LPE, SH, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, d.P, d.E, d.recs, d.mt, d.liab, io, fa);
    return hipGetLastError();
}
hipError_t launch_env_step_act(const EnvDev& d, const StepIO& io, const FusedAct& fa, uint64_t hc_mask, hipStream_t s) {
    if (!env_step_act_supported(d.P, d.E) || io.act_acc == nullptr || io.obs_acc != nullptr) return hipErrorInvalidValue;
    if (hc_mask && (io.act_off == nullptr || d.P.free_prices)) return hipErrorInvalidValue;
    switch (lanes_per_env(d.P, d.E)) {
        case 16: return launch_step_act_sh<16, DynShape>(d, io, fa, hc_mask, s);
        case 32:
#ifndef MS_NO_FIXED_SHAPES
            if (is_shape<4, 4, 3, 1>(d.P)) return launch_step_act_sh<32, FixShape<4, 4, 3, 1>>(d, io, fa, hc_mask, s);
#endif
            return launch_step_act_sh<32, DynShape>(d, io, fa, hc_mask, s);
        default: return launch_step_act_sh<64, DynShape>(d, io, fa, hc_mask, s);
    }
}
template <int LPE, class SH>
static hipError_t launch_rollout_act_sh(const EnvDev& d, const RolloutArgs& A, uint64_t hc_mask, hipStream_t s) {
    constexpr int G = kWave / LPE;
    const int64_t blocks = (d.E + G - 1) / G;
    const size_t lds = (size_t)d.P.s_total * G > 4 * kMtN ? (size_t)d.P.s_total * G : 4 * kMtN;  // >= one MT block
    if (hc_mask) {  // a mixed population (ms_env_rollout_act_mixed)
        const RolloutMixArgs M{A, hc_mask};
        auto kern = A.io.metrics ? k_env_rollout_act_mixed<LPE, SH, true> : k_env_rollout_act_mixed<LPE, SH, false>;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, M);
        return hipGetLastError();
    }
    auto kern = A.io.metrics ? k_env_rollout_act<LPE, SH, true> : k_env_rollout_act<LPE, SH, false>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(kWave), lds, s, A);
    return hipGetLastError();
}
hipError_t launch_env_rollout_act(const EnvDev& d, const StepIO& io, const FusedAct& fa, const RoundStride& st,
                                  int n_rounds, int act_last, uint64_t hc_mask, hipStream_t s) {
    if (!env_step_act_supported(d.P, d.E) || io.act_acc == nullptr || io.obs_acc != nullptr || io.ev_acc != nullptr ||
        io.ev_term != nullptr || n_rounds < 1)
        return hipErrorInvalidValue;
    if (hc_mask && (io.act_off == nullptr || d.P.free_prices)) return hipErrorInvalidValue;
    const RolloutArgs A{d.P, d.E, d.recs, d.mt, d.liab, io, fa, st, n_rounds, act_last};
    switch (lanes_per_env(d.P, d.E)) {
        case 16: return launch_rollout_act_sh<16, DynShape>(d, A, hc_mask, s);
        case 32:
#ifndef MS_NO_FIXED_SHAPES
            if (is_shape<4, 4, 3, 1>(d.P)) return launch_rollout_act_sh<32, FixShape<4, 4, 3, 1>>(d, A, hc_mask, s);
#endif
            return launch_rollout_act_sh<32, DynShape>(d, A, hc_mask, s);
        default: return launch_rollout_act_sh<64, DynShape>(d, A, hc_mask, s);
    }
}
// RolloutFreeArgs::prio: the paced acting (wait after acting 9.0k -> 4.5k cycles, 47.07 -> 46.66 us per round against
// waves 4.. at raised priority for the whole acting, profiles/r7; that 49.6 -> 49.0 against none, profiles/r7c)
constexpr int kFreePrio = 4, kFreeSeparate = 1;
template <class SH>
static hipError_t launch_rollout_free_sh(const RolloutFreeArgs& A, hipStream_t s) {
    const int64_t epb = (int64_t)kFreeEPW * A.P.N;
    const int64_t blocks = (A.E + epb - 1) / epb;
    // MS_FREE_STAGGER=0 (read at every launch; a captured launch keeps what it was captured with): the plain
    // kernel, the tests' reference. Otherwise the staggered one (17.26 -> 16.48 ms per cfg3 iteration,
    // profiles/r10a).
    const char* sv = getenv("MS_FREE_STAGGER");
    const bool stagger = !(sv && strcmp(sv, "0") == 0);
    auto kern = stagger ? (A.io.metrics ? k_env_rollout_act_free<SH, true, true> : k_env_rollout_act_free<SH, false, true>)
                        : (A.io.metrics ? k_env_rollout_act_free<SH, true> : k_env_rollout_act_free<SH, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(64 * A.P.N), (size_t)free_lds(A.P).total, s, A);
    return hipGetLastError();
}
hipError_t launch_env_rollout_act_free(const EnvDev& d, const StepIO& io, const FusedActFree& fa,
                                       const RoundStrideFree& st, const OffCompact& oc, int n_rounds, int act_last,
                                       hipStream_t s) {
    if (!env_rollout_free_supported(d.P) || io.act_acc == nullptr || io.obs_acc != nullptr || io.ev_acc != nullptr ||
        io.ev_term != nullptr || n_rounds < 1 || (oc.tmpl == nullptr) != (oc.pair == nullptr))
        return hipErrorInvalidValue;
    const RolloutFreeArgs A{d.P, d.E, d.recs, d.mt, d.liab, io, fa, st, n_rounds, act_last, kFreePrio, kFreeSeparate,
                            oc};
#ifndef MS_NO_FIXED_SHAPES
    if (is_shape<8, 8, 3, 1>(d.P)) return launch_rollout_free_sh<FixShape<8, 8, 3, 1>>(A, s);
#endif
    return launch_rollout_free_sh<DynShape>(A, s);
}
}  // namespace ms

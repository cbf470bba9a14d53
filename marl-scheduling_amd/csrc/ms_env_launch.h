// ms_env_launch.h — the env launchers (env_kernels.hip, acc_fill_kernels.hip) as capi.cpp calls them, and the
// host-side choices more than one of them makes and capi.cpp asks about: the lane-group width of a launch, the
// shapes with a kernel compiled for their geometry, and the shapes the fused step + act kernels and the
// free-price rollout take.
#pragma once

#include <hip/hip_runtime.h>

#include "ms_layout.h"

namespace ms {

// lanes per env: the smallest power of two >= max(C, N) and >= 16 (a 16-word MT window), so a
// wave steps 4 (cfg2/cfg3), 2 (cfg4) or 1 (cfg5) envs
#ifndef MS_MIN_LPE
#define MS_MIN_LPE 16
#endif
// A launch of >= 1024 replicas in fewer than kEnvMinWaves waves (two per SIMD) widens the lane groups up to
// that many waves, so the chip's SIMDs each hold two waves
// whose waits can hide each other: cfg2 (4096 replicas, 4 x 4) runs 32 lanes per env, 2048 waves,
// instead of 16 lanes, 1024 waves (one per SIMD, every wait exposed).
constexpr long long kEnvMinWaves = 2048;
inline int lanes_per_env(const Params& P, int64_t E) {
    int need = P.C > P.N ? P.C : P.N;
    int lpe = MS_MIN_LPE;
    while (lpe < need) lpe *= 2;
    while (E >= 1024 && lpe < kWave && (E * lpe + kWave - 1) / kWave < kEnvMinWaves &&
           (E * 2 * lpe + kWave - 1) / kWave <= kEnvMinWaves)
        lpe *= 2;
    return lpe;
}

template <int N, int C, int L, int J>
inline bool is_shape(const Params& P) {
    return P.N == N && P.C == C && P.L == L && P.new_jobs == J;
}

// ms_env_step_act: a wave's acceptor items one per lane (<= 64), its offer rows in 16-row tiles (<= 64) and
// its owned cores' rows in one
inline bool env_step_act_supported(const Params& P, int64_t E) {
    const int epw = kWave / lanes_per_env(P, E);
    return epw * P.N * P.C <= kWave && epw * P.NL <= kWave && epw * P.C <= 16;
}

// ms_env_rollout_act_free: 16 lanes per replica (max(N, C) <= 16), one wave per agent (N <= 8: a 512-lane
// workgroup), the core chooser one k-step with <= 16 actions, the acceptor two k-steps with 17..32 actions
// (k_act_pair<1, 1, 1, 2, 2>'s shapes), the price chooser <= 16 actions, two workgroups' LDS per CU with every
// wave's MT twist inside bytes no other wave uses (ms_layout.h)
inline bool env_rollout_free_supported(const Params& P) {
    return P.free_prices && free_rollout_shape_ok(P) && free_rollout_lds_ok(P);
}

// ---- env_kernels.hip (the kernels take d's fields one by one)
// seeds every replica's MT19937 from seed (CPython's init_by_array) and spawns its first jobs
hipError_t launch_env_init(const EnvDev& d, uint64_t seed, hipStream_t s);
// the observations of the current state into io.obs_* (each may be NULL); nothing else of io is read
hipError_t launch_env_reset(const EnvDev& d, const StepIO& io, hipStream_t s);
// one round; mix: the agents that play the rules and where the actions the round used go (MixIO{}: none)
hipError_t launch_env_step(const EnvDev& d, const StepIO& io, const MixIO& mix, hipStream_t s);
// one round and the next round's acting (fixed prices); hc_mask, here and below: the agents that play the rules
hipError_t launch_env_step_act(const EnvDev& d, const StepIO& io, const FusedAct& fa, uint64_t hc_mask, hipStream_t s);
// n_rounds of launch_env_step_act in one launch, round t's arrays st's strides past round 0's
hipError_t launch_env_rollout_act(const EnvDev& d, const StepIO& io, const FusedAct& fa, const RoundStride& st,
                                  int n_rounds, int act_last, uint64_t hc_mask, hipStream_t s);
// the same for a locally shared free-price env; leaves the acceptor items launch_env_fill_common samples.
// oc.tmpl set: compact offer observations every round, io.obs_off's rows by the last round alone (OffCompact{}: rows)
hipError_t launch_env_rollout_act_free(const EnvDev& d, const StepIO& io, const FusedActFree& fa,
                                       const RoundStrideFree& st, const OffCompact& oc, int n_rounds, int act_last,
                                       hipStream_t s);
// random.randrange(n) of replica e's generator into *out (device word)
hipError_t launch_env_randbelow(const EnvDev& d, int64_t e, uint32_t n, uint32_t* out, hipStream_t s);
// the hard-coded auctioneer's actions [E][C] of the current state
hipError_t launch_env_auctioneer(const EnvDev& d, int8_t* actions, hipStream_t s);

// ---- acc_fill_kernels.hip
// an acceptor act fragment block's common-row tables: agent 0's, and the dwords between two agents' tables
void acc_common_tables(const void* act_frag, const uint32_t** tab0, int* group_dwords);
// the acceptor items launch_env_rollout_act_free leaves, with its arguments (of io only obs_cown is read)
hipError_t launch_env_fill_common(const Params& P, int64_t E, const StepIO& io, const FusedActFree& fa,
                                  const RoundStrideFree& st, int n_rounds, int act_last, hipStream_t s);

}  // namespace ms

// ms_env_launch.h — the host-side choices more than one env launcher makes (env_kernels.hip,
// acc_fill_kernels.hip) and capi.cpp asks about: the lane-group width of a launch, the shapes with a kernel
// compiled for their geometry, and the shapes the fused step + act kernels and the free-price rollout take.
#pragma once

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

}  // namespace ms

// act_pair_kernels.hip — ms_act_round_free: both halves of a round's acting in one launch (k_act_pair).
// A translation unit of its own so that this kernel alone builds with LLVM's ILP-first machine scheduler
// (build.sh): the cfg3 rollout 12.14 -> 11.88 ms, while the other acting kernels (cfg4's k_act /
// k_act_common) lose with it (profiles/r3f2). Those live in policy_kernels.hip, built with the default
// scheduler; a round whose shapes have no paired kernel launches them from there (dispatch_act).
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../include/marlsched.h"
#include "ms_act_kernels.h"

#pragma clang fp contract(fast)  // (build.sh: -ffp-contract=fast for this file)

namespace ms {

// getActionForAllAgents of a free-price round (SchedulingEnvironment.py:150-172) in one launch: the
// first off_blocks blocks run the offer units (core + price chooser, k_act), the rest the acceptor
// units on compact rows (k_act_common). The two workloads' waves share the CUs, so one's waits
// hide under the other's work instead of each launch waiting out its own chain.
// (four 4-wave blocks per CU; two for cfg4's acceptor half, whose 128-input rows and 64 action slots take
// ~250 registers)
#ifndef MS_ACT_PAIR_MINB
#define MS_ACT_PAIR_MINB 4
#endif
template <int S1a, int NTa, int NT2a, int S1b, int NTb>
__global__ void __launch_bounds__(256, (S1b >= 4 ? 2 : MS_ACT_PAIR_MINB)) k_act_pair(ActArgs off, ActArgs acc, int off_blocks) {
    if ((int)blockIdx.x < off_blocks)
        act_tiles<S1a, NTa, NT2a, false>(off, blockIdx.x);
    else
        act_common_rows<S1b, NTb, false, true>(acc, (int)blockIdx.x - off_blocks);
}

// both halves of a free-price round's acting in one launch when their shapes have a paired kernel
// (cfg3: offer rows of <= 32 bytes, <= 16 actions; acceptor rows of <= 64 bytes, <= 32 actions),
// else the two launches in order
hipError_t launch_act_round(ActArgs& o, ActArgs& c, hipStream_t st) {
    if (!c.common || !c.owner || c.stride < 16 || c.n_cores < 1 || c.U % c.n_cores != 0) return hipErrorInvalidValue;
    // one replica count; k_act_pair draws its own uniforms (EXT_U false)
    if (o.E < 1 || c.E != o.E || o.uniforms || c.uniforms) return hipErrorInvalidValue;
    const bool price = o.n2.n_groups > 0;
    const int s1a = s1_bucket(o.stride), nta = nt_bucket(o.n1.n_actions);
    const int s1b = s1_bucket(c.stride), ntb = nt_bucket(c.n1.n_actions);
    const bool unpaired = env_int("MS_ACT_UNPAIRED", 0) != 0;
    if (!price) {
        // a fixed-price round (cfg2): the offer units' one net (ActorCritic.act, k_act's single-net body) and the
        // compact acceptors in one launch
        if (s1a != 1 || nta != 1 || s1b != 1 || ntb != 1 || unpaired) {
            hipError_t e = dispatch_act(o, st);
            return e != hipSuccess ? e : dispatch_act(c, st);
        }
        if (!act_tiles_fits(o) || !act_common_fits(c)) return hipErrorInvalidValue;
        // wave split swept at cfg2 (profiles/r5g): 2048 offer / 512 acceptor target waves 8.5 us per launch (two
        // launches: 13.4 us; 1024 / 512: 8.8, 512 / 256: 9.4, 3072 / 512: 11.6, 2048 / 256: 10.8)
        static const long long f_off = env_int("MS_ACT_FIXED_WAVES", 2048), f_acc = env_int("MS_ACT_FIXED_COMMON_WAVES", 512);
        const unsigned ob = act_blocks(o, f_off), cb = act_common_blocks(c, f_acc);
        hipLaunchKernelGGL((k_act_pair<1, 1, 0, 1, 1>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
        return hipGetLastError();
    }
    if (o.n2.in_dim != 4) return hipErrorInvalidValue;
    const bool price16 = nt_bucket(o.n2.n_actions) == 1 && !unpaired;
    const bool paired = s1a == 1 && nta == 1 && s1b == 2 && (ntb == 1 || ntb == 2) && price16;
    // cfg4's shapes (16 x 16 divided): 34-byte offer rows, 17 core actions, 99-byte acceptor rows, 49 actions
    const bool paired4 = s1a == 2 && (nta == 1 || nta == 2) && s1b == 4 && ntb != 0 && ntb <= 4 && price16;
    if (!paired && !paired4) {
        hipError_t e = dispatch_act(o, st);
        return e != hipSuccess ? e : dispatch_act(c, st);
    }
    if (!act_tiles_fits(o) || !act_common_fits(c)) return hipErrorInvalidValue;
    if (paired4) {
        // wave split swept at cfg4 (profiles/r6l, r6m): 1536 offer / 768 acceptor target waves 74.8 us per launch
        // (2048 / 1024: 80.3, 1024 / 1024: 78.4, 3072 / 1536: 78.2, 4096 / 1024: 84.3; two launches: 102.4)
        static const long long f4o = env_int("MS_ACT_PAIR4_WAVES", 1536), f4a = env_int("MS_ACT_PAIR4_COMMON_WAVES", 768);
        const unsigned ob = act_blocks(o, f4o), cb = act_common_blocks(c, f4a);
        hipLaunchKernelGGL((k_act_pair<2, 2, 1, 4, 4>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
        return hipGetLastError();
    }
    // fewer, longer waves than either launch alone: the other half's waves fill the gaps
    // (the tools/gpu_job.sh waves step; profiles/r4af: 2048 / 768 -> 2048 offer and 2048 acceptor waves at cfg3)
    static const long long t_off = env_int("MS_ACT_PAIR_WAVES", 2048), t_acc = env_int("MS_ACT_PAIR_COMMON_WAVES", 768);
    const unsigned ob = act_blocks(o, t_off), cb = act_common_blocks(c, t_acc);
    hipLaunchKernelGGL((k_act_pair<1, 1, 1, 2, 2>), dim3(ob + cb), dim3(256), 0, st, o, c, (int)ob);
    return hipGetLastError();
}

#ifdef MS_ACT_PROBE
// profiling build only: the paired act kernel's per-phase cycles, out[2][17] (the last column: waves)
extern "C" int ms_probe_act_cycles(unsigned long long* out, int clear) {
    static unsigned long long cyc[2][kActProbeWaves][16], waves[2][kActProbeWaves];
    if (hipMemcpyFromSymbol(cyc, HIP_SYMBOL(g_act_cycles), sizeof(cyc)) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(waves, HIP_SYMBOL(g_act_waves), sizeof(waves)) != hipSuccess) return -1;
    for (int h = 0; h < 2; h++) {
        for (int k = 0; k < 17; k++) out[17 * h + k] = 0;
        for (int w = 0; w < kActProbeWaves; w++) {
            for (int k = 0; k < 16; k++) out[17 * h + k] += cyc[h][w][k];
            out[17 * h + 16] += waves[h][w];
        }
    }
    if (clear) {
        memset(cyc, 0, sizeof(cyc));
        memset(waves, 0, sizeof(waves));
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_act_cycles), cyc, sizeof(cyc)) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_act_waves), waves, sizeof(waves)) != hipSuccess) return -1;
    }
    return 0;
}
#endif

}  // namespace ms

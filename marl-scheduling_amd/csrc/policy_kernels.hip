// policy_kernels.hip — PPO action selection (sampling) for gfx950.
//
// k_act: ActorCritic.act (PPOmodules.py:53-63) for every unit of every env
// replica. A wave takes 16 observation rows at a time and runs
// Linear(D,16)-tanh-Linear(16,16)-tanh-Linear(16,A) with the batch on the MFMA
// column (lane) axis, so each layer's accumulator is the next layer's B operand
// unchanged. Layer 1 is three v_mfma_f32_16x16x32_bf16 per 32 inputs: the int8
// observations are exact in bf16 and the f32 weights are split into three bf16
// terms that sum to them exactly (error of the f32 accumulation only); layers
// 2-3 run on v_mfma_f32_16x16x4_f32 with the weights read in a permuted k order.
// All weights live in registers; the kernel uses no LDS. Softmax, the
// Categorical renormalisation and the inverse-CDF sample run on the accumulator
// layout: a row's logits live in 4 lanes x 4 registers per 16 actions.
// With a second (price) net the kernel is FreePriceOfferPPO.selectAction
// (PPOmodules.py:312-332): core chooser, then the price chooser on
// [obs[2a:2a+2], obs[-2:]] (or the dummy [-5,-5,-5,-5] for a = 0), in one launch.
//
// k_act_common: the same for rows that mostly equal one common row. Both kernels' bodies are in
// ms_act_kernels.h (act_tiles, act_common_rows), which k_act_pair (act_pair_kernels.hip) runs side by
// side in one launch; dispatch_act here is the one place that launches k_act / k_act_common.
// k_act_prep: the weights as the acting waves hold them, made once per weight update (ms_act_prepare).
// k_price_table: the price chooser's sampling table (ms_price_table_build).
// (The greedy kernels are in greedy_kernels.hip, the returns in returns_kernels.hip.)
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/marlsched.h"
#include "ms_act_kernels.h"

#pragma clang fp contract(fast)  // (build.sh: -ffp-contract=fast for this file)

namespace ms {

template <int S1, int NT, int NT2, bool EXT_U>
__global__ void __launch_bounds__(256) k_act(ActArgs a) {
    act_tiles<S1, NT, NT2, EXT_U, true>(a, blockIdx.x);
}

template <int S1, int NT, bool EXT_U, bool OWN>
__global__ void __launch_bounds__(256) k_act_common(ActArgs a) {
    act_common_rows<S1, NT, EXT_U, OWN, true>(a, blockIdx.x);
}

template <int S1, int NT>
static hipError_t launch_act_common_t(ActArgs& a, hipStream_t st) {
    if (!act_common_fits(a)) return hipErrorInvalidValue;
    auto kern = a.owner ? (a.uniforms ? k_act_common<S1, NT, true, true> : k_act_common<S1, NT, false, true>)
                        : (a.uniforms ? k_act_common<S1, NT, true, false> : k_act_common<S1, NT, false, false>);
    static const long long target = env_int("MS_ACT_COMMON_WAVES", 1536);  // measured best for cfg3 alone
    const unsigned blocks = act_common_blocks(a, target);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int S1, int NT, int NT2>
static hipError_t launch_act_t(ActArgs& a, hipStream_t st) {
    if (!act_tiles_fits(a)) return hipErrorInvalidValue;
    auto kern = a.uniforms ? k_act<S1, NT, NT2, true> : k_act<S1, NT, NT2, false>;
    static const long long target = env_int("MS_ACT_WAVES", 8192);  // measured best for cfg3 alone
    const unsigned blocks = act_blocks(a, target);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

template <int S1>
static hipError_t dispatch_act_s(ActArgs& a, hipStream_t st) {
    const bool two = a.n2.n_groups > 0;
    const int nt = nt_bucket(a.n1.n_actions), nt2 = two ? nt_bucket(a.n2.n_actions) : 0;
#define MS_ACT(T, T2) \
    case T: return launch_act_t<S1, T, T2>(a, st);
    if (a.common && a.stride >= 16) {
        if (two) return hipErrorInvalidValue;
        switch (nt) {
            case 1: return launch_act_common_t<S1, 1>(a, st);
            case 2: return launch_act_common_t<S1, 2>(a, st);
            case 4: return launch_act_common_t<S1, 4>(a, st);
            case 8: return launch_act_common_t<S1, 8>(a, st);
        }
    } else if (!two) {
        switch (nt) { MS_ACT(1, 0) MS_ACT(2, 0) MS_ACT(4, 0) MS_ACT(8, 0) }
    } else if (nt2 == 1) {
        switch (nt) { MS_ACT(1, 1) MS_ACT(2, 1) MS_ACT(4, 1) }
    } else if (nt2 == 2) {
        switch (nt) { MS_ACT(1, 2) MS_ACT(2, 2) MS_ACT(4, 2) }
    } else if (nt2 != 0) {  // 3 to 8 price tiles: one variant
        if (nt != 0 && nt <= 4) return launch_act_t<S1, 4, 8>(a, st);
    }
#undef MS_ACT
    return hipErrorInvalidValue;
}

hipError_t dispatch_act(ActArgs& a, hipStream_t st) {
    if (a.E < 1 || (a.n2.n_groups > 0 && a.n2.in_dim != 4)) return hipErrorInvalidValue;
    // compact rows are k_act_common's alone: they need the common row, and the units split into agents' cores
    if (a.owner && (!a.common || a.stride < 16 || a.n_cores < 1 || a.U % a.n_cores != 0)) return hipErrorInvalidValue;
    switch (s1_bucket(a.stride)) {
        case 1: return dispatch_act_s<1>(a, st);
        case 2: return dispatch_act_s<2>(a, st);
        case 4: return dispatch_act_s<4>(a, st);
        case 8: return dispatch_act_s<8>(a, st);
    }
    return hipErrorInvalidValue;
}

// ms_act_prepare: one wave per group writes each lane's fragment (what the acting waves would derive:
// W1Split::load, Head::load) and, with a common row, its sampling table (common_table: the same
// arithmetic as the acting waves', so acting with the block is bit-identical to acting without).
template <int S1, int NT>
__global__ void __launch_bounds__(64) k_act_prep(ms_mlp_params p, const int8_t* common, int stride, uint32_t* frag) {
    using FL = FragLayout<S1, NT>;
    __shared__ uint32_t tmpl[8 * S1];
    __shared__ float cum[16 * NT], lp[16 * NT], S;
    __shared__ int lnz;
    const int grp = blockIdx.x, lane = threadIdx.x, j = lane & 15, g4 = lane >> 4;
    W1Split<S1> w1;
    w1.load(p.w1 + (size_t)grp * 16 * p.in_dim, p.in_dim, j, g4);
    Head<NT, true> h1;  // the tables' zero numerators: Head's ZFIX
    h1.load(p, grp, j, g4);
    uint32_t* gb = frag + 4 + (size_t)grp * FL::GB;
    w1.store_frag(gb + lane * FL::LW);
    h1.store_frag(reinterpret_cast<float*>(gb + lane * FL::LW + 12 * S1));
    if (common) {
        common_table<S1, NT>(w1, h1, common, stride >> 2, tmpl, cum, lp, &S, &lnz, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        uint32_t* tb = gb + 64 * FL::LW;
        for (int k = lane; k < FL::TB; k += 64)
            tb[k] = k < 16 * NT ? __float_as_uint(cum[k])
                                : (k < 32 * NT ? __float_as_uint(lp[k - 16 * NT])
                                               : (k == 32 * NT ? __float_as_uint(S) : (k == 32 * NT + 1 ? (uint32_t)lnz : 0u)));
    }
    if (grp == 0 && lane < 4)
        frag[lane] = lane == 0 ? kFragMagic : (lane == 1 ? (uint32_t)S1 : (lane == 2 ? (uint32_t)NT : (common ? 1u : 0u)));
}

size_t act_frag_bytes(const ms_mlp_params* p, int stride) {
    const int s1 = s1_bucket(stride), nt = nt_bucket(p->n_actions);
    if (!s1 || !nt) return 0;
    const int lw = 12 * s1 + 12 + 8 * nt, gb = 64 * lw + 32 * nt + 4;
    return 4 * (4 + (size_t)p->n_groups * gb);
}

template <int S1>
static hipError_t launch_act_prep_s(const ms_mlp_params* p, const int8_t* common, int stride, uint32_t* frag, int nt,
                                    hipStream_t st) {
    const dim3 grid((unsigned)p->n_groups);
    switch (nt) {
        case 1: hipLaunchKernelGGL((k_act_prep<S1, 1>), grid, dim3(64), 0, st, *p, common, stride, frag); break;
        case 2: hipLaunchKernelGGL((k_act_prep<S1, 2>), grid, dim3(64), 0, st, *p, common, stride, frag); break;
        case 4: hipLaunchKernelGGL((k_act_prep<S1, 4>), grid, dim3(64), 0, st, *p, common, stride, frag); break;
        default: hipLaunchKernelGGL((k_act_prep<S1, 8>), grid, dim3(64), 0, st, *p, common, stride, frag); break;
    }
    return hipGetLastError();
}

hipError_t launch_act_prepare(const ms_mlp_params* p, const int8_t* common, int stride, void* frag, hipStream_t st) {
    const int s1 = s1_bucket(stride), nt = nt_bucket(p->n_actions);
    if (!s1 || !nt || p->hidden != 16) return hipErrorInvalidValue;
    uint32_t* f = static_cast<uint32_t*>(frag);
    switch (s1) {
        case 1: return launch_act_prep_s<1>(p, common, stride, f, nt, st);
        case 2: return launch_act_prep_s<2>(p, common, stride, f, nt, st);
        case 4: return launch_act_prep_s<4>(p, common, stride, f, nt, st);
        default: return launch_act_prep_s<8>(p, common, stride, f, nt, st);
    }
}

// The price chooser's sampling table (ms_price_table_build): the forward of every tabulated 4-byte
// input per group (16 keys per tile, one per column), stored as Head::run would use it.
template <int NT2>
__global__ void __launch_bounds__(256) k_price_table(ms_mlp_params pn, const int8_t* rows, int K, float* tab) {
    constexpr int TW = PriceTW<NT2>::v;
    const int tid = threadIdx.x, lane = tid & 63, j = lane & 15, g4 = lane >> 4;
    const int gw = blockIdx.x * 4 + (tid >> 6);
    const int tiles = (K + 15) / 16;
    const int grp = gw / tiles, tile = gw - grp * tiles;
    if (grp >= pn.n_groups) return;
    Head<NT2, true> h;
    h.load(pn, grp, j, g4);
    const float pw1 = pn.w1[((size_t)grp * 16 + j) * 4 + g4];
    const int key = 16 * tile + j;
    const int8_t pin = rows[(size_t)min(key, K - 1) * 4 + g4];
    f4 acc = {0, 0, 0, 0};
    acc = mfma4(pw1, (float)pin, acc);
    float c[NT2][4], lp[NT2][4], S;
    int lnz;
    h.row_table(acc, g4, c, lp, S, lnz);
    if (key < K) {
        float* te = tab + ((size_t)grp * K + key) * TW;
#pragma unroll
        for (int t = 0; t < NT2; t++)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                te[16 * t + 4 * g4 + q] = c[t][q];
                te[16 * NT2 + 16 * t + 4 * g4 + q] = lp[t][q];
            }
        if (g4 == 0) {
            te[32 * NT2] = S;
            te[32 * NT2 + 1] = __int_as_float(lnz);
        }
    }
}

hipError_t launch_price_table(const ms_mlp_params* pn, const int8_t* rows, int K, float* tab, hipStream_t st) {
    if (pn->in_dim != 4 || pn->hidden != 16 || K < 1) return hipErrorInvalidValue;
    const int nt = (pn->n_actions + 15) / 16;
    const long long waves = (long long)pn->n_groups * ((K + 15) / 16);
    const dim3 grid((unsigned)((waves + 3) / 4));
    if (nt <= 1)
        hipLaunchKernelGGL(k_price_table<1>, grid, dim3(256), 0, st, *pn, rows, K, tab);
    else if (nt <= 2)
        hipLaunchKernelGGL(k_price_table<2>, grid, dim3(256), 0, st, *pn, rows, K, tab);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace ms

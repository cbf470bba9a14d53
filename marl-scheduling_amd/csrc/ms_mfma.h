// ms_mfma.h — the small numeric primitives every MFMA kernel of the library shares, defined once: the MFMA
// wrappers and their fragment types, the bf16 packing, the exact three-term bf16 split, and the fast
// transcendentals of the acting nets. The act kernels (ms_act.h), the PPO gradient's regenerating scan
// (ppo_kernels.hip) and the Branching-DQN kernels include it; the act kernels and the gradient must agree
// bit for bit (tests/test_acc_regen_gpu.py), which is why there is one copy.
//
// The header sets no floating-point contraction of its own: everything here is force-inlined and takes the
// includer's mode, as the includers' own copies did. ms_act.h includes it after its contract(fast) pragma
// (so the env units, built with contraction off, get the act kernels' rounding); ppo_kernels.hip and
// bdqn_kernels.hip compile under -ffp-contract=on, bdqn_update_kernels.hip under off (build.sh).
// A unit that uses ms_act.h gets this header through it and never includes it first: after #pragma once the
// primitives the act code calls would otherwise take the command line's mode, not contract(fast), and the act
// kernels of that unit would no longer match the others bit for bit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ms {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4 mfma4(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f4 mfma_bf16(const u4v& a, const u4v& b, f4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0,
                                                   0);
}

// tanh(x) = 1 - 2 / (1 + exp(2x)): exp overflows to inf for large x (-> 1) and underflows to 0 for
// large -x (-> -1); absolute error ~1e-7 (what feeds the next layers' sums of O(1) terms).
// tanh(a + b) with the bias pre-scaled, bs = b * 2 log2(e) (kTanhScale): the exponent is one fma
constexpr float kTanhScale = 2.8853900817779268f;
__device__ __forceinline__ float fast_tanh_b(float a, float bs) {
    const float t = __builtin_amdgcn_exp2f(fmaf(a, kTanhScale, bs));  // exp(2(a + b))
    return fmaf(-2.f, __builtin_amdgcn_rcpf(1.f + t), 1.f);
}
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
// exp(x - m) as exp2(x log2e - m log2e) with one fma (m_l2e = m * log2e)
__device__ __forceinline__ float fast_exp_sub(float x, float m_l2e) {
    return __builtin_amdgcn_exp2f(fmaf(x, 1.4426950408889634f, -m_l2e));
}
__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * 0.69314718055994531f; }

// bf16 (upper half of the f32 bits) of elements 2i, 2i+1 packed into one dword
__device__ __forceinline__ uint32_t pack_hi(float lo, float hi) {
    return __builtin_amdgcn_perm(__float_as_uint(hi), __float_as_uint(lo), 0x07060302u);  // one v_perm_b32
}
__device__ __forceinline__ float trunc_bf16(float x) { return __uint_as_float(__float_as_uint(x) & 0xffff0000u); }

// 8 floats as three bf16 fragments with v = hi + mid + lo exactly (truncation leaves exact residuals:
// each term keeps 8 significant bits)
__device__ __forceinline__ void split3(const float (&v)[8], u4v& hi, u4v& mid, u4v& lo) {
#pragma unroll
    for (int d = 0; d < 4; d++) {
        float h[2], m[2], l[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            h[t] = trunc_bf16(v[2 * d + t]);
            const float r = v[2 * d + t] - h[t];
            m[t] = trunc_bf16(r);
            l[t] = r - m[t];
        }
        hi[d] = pack_hi(h[0], h[1]);
        mid[d] = pack_hi(m[0], m[1]);
        lo[d] = pack_hi(l[0], l[1]);
    }
}

// int8 values (exact in bf16) packed in pairs
__device__ __forceinline__ uint32_t pack_i8(int a, int b) { return pack_hi((float)a, (float)b); }
// int8 observation bytes (two dwords = 8 consecutive inputs) as a bf16 B fragment (exact)
__device__ __forceinline__ u4v bytes_to_bf16(uint32_t d0, uint32_t d1) {
    u4v r;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        const uint32_t src = d < 2 ? d0 : d1;
        const int sh = 16 * (d & 1);
        const float a = (float)(int8_t)(src >> sh);
        const float b = (float)(int8_t)(src >> (sh + 8));
        r[d] = pack_hi(a, b);
    }
    return r;
}

}  // namespace ms

// The split-f16 operand format of the conv kernels, and the few definitions every one of them needs -- written once.
// Users: conv_rl16, conv_rb16, conv_ou16, conv_oc16, conv_up16, conv_mfma (conv_sk16 / conv_gv16), and the f32 conv_rl for
// act_in, buf_load4 and the typedefs.
//
// Every f32 operand is carried as two f16 numbers
//     v = hi + lo / 2048,   hi = f16(v),   lo = f16((v - hi) * 2048)          (22+ significant bits)
// and a product sum is formed from three v_mfma_f32_32x32x16_f16 per 16 k:
//     acc0 += A_hi * B_hi          acc1 += A_hi * B_lo + A_lo * B_hi          result = acc0 + acc1 / 2048
// f16 x f16 products are exact in the f32 accumulator, so the only errors are the dropped lo*lo term
// (2^-22 relative) and the 2^-22 representation error of each operand -- measured on gfx950 against fp64
// (tools/mfma_f16_probe.hip, profiles/r1_f16_split_probe.txt): max |err| / sum|a b| = 8e-8 for K = 352..2816,
// BELOW the 2e-7 of the f32 MFMA chain (which rounds after every product), at 3/16 of its matrix-core time.
// f16 subnormal inputs are honoured by the instruction (same probe); |v| > 65504 overflows hi to inf, which makes every
// output it feeds non-finite -- the epilogues test their outputs (not_finite4) and raise device flag bit 3 (adk_debug_flags).
// Weights come pre-split in fragment order (adk_pack_weights_split16).
//
// Only definitions and expressions live here.  The MFMA loops stay in their kernels, with their loads: hipcc schedules a loop
// that sits in a helper differently (ds_reads move, waits appear), and these kernels count their waits by hand.
#pragma once
#include "adk_common.h"
#include <type_traits>

namespace adk {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef const void __attribute__((address_space(1)))* gptr_t;
typedef void __attribute__((address_space(3)))* lptr_t;
typedef unsigned char __attribute__((address_space(3)))* lds_u8_t;

constexpr float kLoScale = 2048.f, kLoInv = 1.f / 2048.f;

// input activation of a conv, chosen at compile time (ELU / LeakyReLU / none)
template <int ACT>
__device__ __forceinline__ float act_in(float x, float slope) {
    if (ACT == ADK_ACT_ELU) return x > 0.f ? x : expm1_neg(x);
    if (ACT == ADK_ACT_LEAKY) return x > 0.f ? x : x * slope;
    return x;
}

// ---- the split: y -> (hi, lo) ----
// element e of a pair of f16 vectors (the statement order is the one every kernel was scheduled with: keep it)
__device__ __forceinline__ _Float16 lo_part(float y, _Float16 hi) { return (_Float16)((y - (float)hi) * kLoScale); }
template <typename V>
__device__ __forceinline__ void split_to(float y, V& hi, V& lo, int e) {
    const _Float16 h = (_Float16)y;
    hi[e] = h;
    lo[e] = lo_part(y, h);
}
// N = 4 or 8 consecutive k of one column: act_in<ACT>, then the split
template <int ACT, int N, typename V>
__device__ __forceinline__ void act_split(const float (&x)[N], float slope, V& hi, V& lo) {
#pragma unroll
    for (int e = 0; e < N; ++e) split_to(act_in<ACT>(x[e], slope), hi, lo, e);
}
template <int ACT>
__device__ __forceinline__ void act_split8(const float4& u, const float4& v, float slope, f16x8& hi, f16x8& lo) {
    const float x[8] = {u.x, u.y, u.z, u.w, v.x, v.y, v.z, v.w};
    act_split<ACT>(x, slope, hi, lo);
}
template <int ACT>
__device__ __forceinline__ void act_split4(const float4& v, float slope, f16x4& hi, f16x4& lo) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    act_split<ACT>(x, slope, hi, lo);
}
__device__ __forceinline__ void split8(const float4& u, const float4& v, f16x8& hi, f16x8& lo) { act_split8<ADK_ACT_NONE>(u, v, 0.f, hi, lo); }

// ---- the join: main + cross / 2048, one accumulator element or four; and the test of what comes out ----
__device__ __forceinline__ float join(float main, float cross) { return fmaf(cross, kLoInv, main); }
__device__ __forceinline__ float4 join4(const f32x4& am, const f32x4& ac) {
    return make_float4(join(am[0], ac[0]), join(am[1], ac[1]), join(am[2], ac[2]), join(am[3], ac[3]));
}
__device__ __forceinline__ float4 join4(const f32x16& am, const f32x16& ac, int qd) {      // quad qd of a 32 x 32 accumulator
    return make_float4(join(am[4 * qd], ac[4 * qd]), join(am[4 * qd + 1], ac[4 * qd + 1]), join(am[4 * qd + 2], ac[4 * qd + 2]), join(am[4 * qd + 3], ac[4 * qd + 3]));
}
// an operand beyond the f16 range was split into inf parts: every output it feeds is inf or NaN
__device__ __forceinline__ bool not_finite(float x) { return !(fabsf(x) <= 3.0e38f); }
__device__ __forceinline__ bool not_finite4(const float4& v) { return not_finite(v.x) | not_finite(v.y) | not_finite(v.z) | not_finite(v.w); }

__device__ __forceinline__ f16x8 as_f16x8(const u32x4& v) {
    union { u32x4 u; f16x8 h; } c; c.u = v; return c.h;
}
__device__ __forceinline__ float4 buf_load4(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}

// LDS-DMA of 16 bytes per lane (global_load_lds_dwordx4: lane i's bytes land at m0val + 16 i).  The compiler does not see the load:
// whoever reads what it brings counts the wait (wait_vm).  M0 is the compiler's: put back.
#define ADK_LDS_DMA16(gptr, m0val) do { unsigned m0_keep_; asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" \
                                                                 : "=&s"(m0_keep_) : "v"(gptr), "s"(m0val) : "memory"); } while (0)
// at most N of this wave's vector-memory instructions still in flight
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N <= 63, "vmcnt is six bits");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// ---- host side ----
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// what 16-byte accesses along the channel axis need of a conv's tensors: in / out / wfrag (and bias, residual where present) 16-byte
// aligned, channel counts, offsets and group strides multiples of 4
inline bool conv_io_aligned(const ConvArgs& a) {
    if ((a.in_ch % 4) || (a.in_choff % 4) || (a.in_gstride % 4) || (a.out_ch % 4) || (a.out_choff % 4)) return false;
    if (!aligned16(a.in) || !aligned16(a.out) || !aligned16(a.wfrag) || (a.bias && !aligned16(a.bias))) return false;
    if (a.res && ((a.res_ch % 4) || (a.res_choff % 4) || (a.res_gstride % 4) || !aligned16(a.res))) return false;
    return true;
}

// f(std::integral_constant<int, ACT>()) for the input activation `act` (ELU / LeakyReLU / none).  Any other value fails with
// `unsupported` -- or, unsupported == nullptr, runs as "none" (launchers whose *_fusable test has seen the value).
template <typename F>
int with_act_in(int act, const char* unsupported, F&& f) {
    if (act == ADK_ACT_ELU) return f(std::integral_constant<int, ADK_ACT_ELU>());
    if (act == ADK_ACT_LEAKY) return f(std::integral_constant<int, ADK_ACT_LEAKY>());
    if (act == ADK_ACT_NONE || !unsupported) return f(std::integral_constant<int, ADK_ACT_NONE>());
    return fail(ADK_ERR_ARG, unsupported);
}

}  // namespace adk

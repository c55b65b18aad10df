// gguf_attn.hpp -- what attn_decode.hip and attn_prefill.hip share beside the arithmetic they describe
// in their headers: the fp16 LDS swizzle, the exp2-domain helpers and the soft-cap with its constants.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gq {

constexpr float kLog2e = 1.4426950408889634f;

// fp16 tile rows: piece p of row r sits at piece p ^ f16_swz<D>(r) (attn_decode.hip has the bank argument)
template <int D> __device__ __forceinline__ int f16_swz(int r) { return D == 64 ? ((r >> 1) & 7) : (r & 15); }

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float xor_lanes(float v, int m) { return __shfl_xor(v, m, 64); }

// Soft-cap in the exp2 domain: cap * tanh(scale s / cap) * log2(e) = cc * tanh(x), cc = cap log2(e),
// x = s scale / cap, tanh(x) = 1 - 2 / (1 + 2^t) with t = 2 log2(e) x = s * cx.  One v_exp_f32, one
// v_rcp_f32, one fma; t -> +-inf gives +-cc exactly.  Absolute error of the tanh below 2^-21.
struct SoftCap {
    float cx = 0.f, cc = 0.f;
};
inline SoftCap softcap_consts(float scale, float cap) { return SoftCap{2.f * kLog2e * scale / cap, cap * kLog2e}; }
__device__ __forceinline__ float capped(float t, float cc) { return __builtin_fmaf(-2.f * cc, __builtin_amdgcn_rcpf(1.f + ex2(t)), cc); }

} // namespace gq

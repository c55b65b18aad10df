// gguf_rope.hpp -- what rope.hip and attn_mla.hip share: the rotation's angle with its sin/cos (rope.hip's
// header has the arithmetic) and the two-element row accesses.
#pragma once
#include "gguf_blocks.hpp"

namespace gq {

// (m cos, m sin) of theta = p * f
__device__ __forceinline__ void rope_cs(int p, float f, float m, float &c, float &s)
{
    const double th = (double)p * (double)f;
    const double q = __builtin_rint(th * 0.63661977236758134308);
    double r = __builtin_fma(-q, 1.57079632679489655800e+00, th);
    r = __builtin_fma(-q, 6.12323399573676603587e-17, r);
    const float x = (float)r, z = x * x;
    float sn = __builtin_fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f);
    sn = __builtin_fmaf(sn, z, -1.6666654611e-1f);
    sn = __builtin_fmaf(sn * z, x, x);
    float cs = __builtin_fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f);
    cs = __builtin_fmaf(cs, z, 4.166664568298827e-2f);
    cs = __builtin_fmaf(cs * z, z, __builtin_fmaf(-0.5f, z, 1.0f));
    const int k = (int)((long long)q & 3);
    const float sk = (k & 1) ? cs : sn, ck = (k & 1) ? sn : cs;
    s = m * ((k & 2) ? -sk : sk);
    c = m * (((k + 1) & 2) ? -ck : ck);
}

// two fp16 of one row at elements e0, e1 (pair: e1 == e0 + 1 and the row takes a 4-byte access)
__device__ __forceinline__ uint32_t load2(const uint16_t *row, int e0, int e1, bool pair)
{
    if (pair) return *(const uint32_t *)(row + e0);
    return (uint32_t)row[e0] | ((uint32_t)row[e1] << 16);
}

__device__ __forceinline__ void store2(uint16_t *row, int e0, int e1, bool pair, uint32_t v)
{
    if (pair) {
        *(uint32_t *)(row + e0) = v;
    } else {
        row[e0] = (uint16_t)v;
        row[e1] = (uint16_t)(v >> 16);
    }
}

} // namespace gq

// gguf_blocks.hpp -- GGUF packed-block layouts and the device-side helpers that read them.
//
// Layouts (little endian; a weight tensor is rows of K/QK consecutive blocks, no padding):
//   Q8_0  32 elems / 34 B : [0:2] d fp16 | [2:34] qs int8[32]               w = d*q
//   Q4_K 256 elems /144 B : [0:2] d | [2:4] dmin | [4:16] 6-bit sc/m x8 | [16:144] qs nibbles
//                           w = d*sc_j*q - dmin*m_j   (sub-block j = e/32)
//   Q6_K 256 elems /210 B : [0:128] ql | [128:192] qh | [192:208] int8 sc x16 | [208:210] d
//                           w = d*sc_{e/16}*(q - 32)
//   Q5_K 256 elems /176 B : [0:2] d | [2:4] dmin | [4:16] 6-bit sc/m x8 (Q4_K's) | [16:48] qh |
//                           [48:176] qs nibbles;  q = nibble + 16*((qh[e%32] >> e/32) & 1)
//                           w = d*sc_j*q - dmin*m_j   (sub-block j = e/32)
//   Q3_K 256 elems /110 B : [0:32] hmask | [32:96] qs (2-bit) | [96:108] 6-bit sc x16 | [108:110] d
//                           q = ((qs[32*(e/128) + e%32] >> 2*((e%128)/32)) & 3)
//                               + 4*((hmask[e%32] >> e/32) & 1) - 4;  w = d*(sc_{e/16} - 32)*q
//   Q2_K 256 elems / 84 B : [0:16] scales (sc = low nibble, m = high, per 16 elements) |
//                           [16:80] qs (2-bit, Q3_K's layout) | [80:82] d | [82:84] dmin
//                           q = (qs[32*(e/128) + e%32] >> 2*((e%128)/32)) & 3;  w = d*sc_{e/16}*q - dmin*m_{e/16}
//   Q4_0  32 elems / 18 B : [0:2] d fp16 | [2:18] qs[16]  (element j: qs[j] & 15, element 16+j: qs[j] >> 4)
//                           w = d*(q - 8)   (a Q8_0 block with the same d and the int8 codes q - 8;
//                           256 weights are 144 bytes, as Q4_K's)
//   Q8_1 (activations) 36 B: [0:2] d | [2:4] s = d*sum(q) | [4:36] qs int8[32]
// Reference: block docs in kernels/mmq_q4_k.py:1-16, kernels/mmq_q6_k.py:1-14,
// utils/quantize/q8_1.py:1-11; unpack rules kernels/mmq_q4_k.py:30-114, mmq_q6_k.py:28-68.
//
// "Unit" = the 64 consecutive-in-K weights one lane of the GEMV owns (two 32-element
// activation blocks).  Every format is read straight from HBM into registers with 16-byte
// loads: gfx950 runs with unaligned global access enabled, so the 2-byte-aligned Q8_0/Q6_K
// fields are loaded as dwordx4 without byte shuffling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace gq {

enum Fmt : int { Q8_0 = 0, Q4_K = 1, Q6_K = 2, Q5_K = 3, Q3_K = 4, Q2_K = 5, Q4_0 = 6 };

// The cached-chunk caps of the Q3_K / Q2_K decode kernels (FmtInfo below), with their build-time
// overrides (make variant VFLAGS=... A/B builds).
constexpr int kQ3Itc1 = 6, kQ3Itc2 = 3; // Q3_K: the most cached chunks at one / two tokens
// Q2_K: Q3_K's activation registers, but 10 raw registers per unit in flight where Q3_K has 20:
// 7 cached chunks at one token compile without scratch (236 VGPRs), as do 4 at two (253); two
// tokens stay at Q3_K's 3, the most the grouped kernel that holds a Q2_K item carries
#ifndef GQ_Q2_ITC1
#define GQ_Q2_ITC1 7
#endif
#ifndef GQ_Q2_ITC2
#define GQ_Q2_ITC2 3
#endif
constexpr int kQ2Itc1 = GQ_Q2_ITC1, kQ2Itc2 = GQ_Q2_ITC2;
// Q4_0: Q8_0's unit registers after the decode (16 code words, two scales) and 10 raw registers
// in flight where Q8_0 has 18: Q8_0's caps compile without scratch
#ifndef GQ_Q40_ITC1
#define GQ_Q40_ITC1 7
#endif
#ifndef GQ_Q40_ITC2
#define GQ_Q40_ITC2 4
#endif
constexpr int kQ40Itc1 = GQ_Q40_ITC1, kQ40Itc2 = GQ_Q40_ITC2;

// What the host side and the kernels' template parameters need to know of a block type: one row
// per Fmt in kFmt[].  A new type is a row here plus its device code ("Adding a block type").
struct FmtInfo {
    int qk, bytes; // elements and bytes of one block
    // Q4_K's header and q8_1 arithmetic (6-bit scales and mins, the activation block's s in the min term)
    bool has_mins;
    // Q6_K's q8_1 arithmetic (a signed scale per 16 elements, no mins; the codes enter v_dot4 unsigned
    // and code_offset -- Q6_K 32, Q3_K 4 -- is taken out with the activations' per-16 code sums)
    // (Q2_K: unsigned codes 0..3 and a min per 16 elements -- the same per-16 code sums carry dmin*m)
    bool has_sums;
    int code_offset;
    // no fp8 activation form and no resident / skinny / K-chunked / LDS-DMA GEMM: only the q8_1
    // decode kernels, the GEMV and the streaming GEMM
    bool q8_1_only;
    // streaming decode (mmq_decode.hip): the most cached activation chunks a kernel exists for, at
    // one / two / four tokens with q8_1 activations and at one token with fp8 ones (unused where
    // q8_1_only), and the 64-weight units of a lane's work item at up to two tokens.
    // (Q5_K: twice Q4_K's code registers per unit -- 7 cached units at one token spill;
    // Q3_K: Q5_K's code registers and the code sums besides)
    int itc[3], fp8_itc, upc2;
    // the case set a grouped launch holding the type needs, the largest over its items:
    // stream_decode_grouped_kernel's SET and sgemm_grouped_kernel's
    int group_set, sgemm_set;
    constexpr int sb_bytes() const { return 256 / qk * bytes; } // the bytes of 256 weights (Q8_0: 272)
};
constexpr FmtInfo kFmt[] = {
    // qk bytes mins   sums   off  q8_1only  itc at 1, 2, 4 tokens  fp8 upc2 sets
    {32, 34, false, false, 32, false, {7, 4, 1}, 2, 1, 0, 0},              // Q8_0
    {256, 144, true, false, 32, false, {7, 4, 1}, 2, 1, 0, 0},             // Q4_K
    {256, 210, false, true, 32, false, {4, 1, 1}, 1, 2, 0, 0},             // Q6_K
    {256, 176, true, false, 32, true, {6, 4, 1}, 2, 1, 1, 0},              // Q5_K
    {256, 110, false, true, 4, true, {kQ3Itc1, kQ3Itc2, 1}, 2, 1, 2, 1},   // Q3_K
    // 84 = 4 * 21 bytes: every super-block and every field is 4-byte aligned
    {256, 84, false, true, 32, true, {kQ2Itc1, kQ2Itc2, 1}, 2, 1, 3, 2},   // Q2_K
    // Q8_0's q8_1 arithmetic on the signed nibbles: no mins, no code sums (code_offset unused)
    {32, 18, false, false, 32, true, {kQ40Itc1, kQ40Itc2, 1}, 2, 1, 4, 3}, // Q4_0
};
constexpr int kNumFmts = (int)(sizeof(kFmt) / sizeof(kFmt[0]));
constexpr bool known_fmt(int f) { return f >= 0 && f < kNumFmts; }
// A type outside the table (every caller refuses it by known_fmt first): Q6_K's block -- the C
// ABI's answer for an unknown type's row size -- with the general caps.
constexpr FmtInfo kFmtOther = {256, 210, false, true, 32, false, {7, 4, 1}, 2, 1, 0, 0};
constexpr const FmtInfo &fmt_info(int f) { return known_fmt(f) ? kFmt[f] : kFmtOther; }
// packed bytes of a K-element row.  Not K / 256 * sb_bytes: a Q8_0 / Q4_0 row may be a multiple of 32 only
constexpr int64_t row_bytes(int f, int64_t K) { return K / fmt_info(f).qk * fmt_info(f).bytes; }

template <int F> struct Layout { static constexpr int QK = kFmt[F].qk, BYTES = kFmt[F].bytes; };
constexpr bool has_mins(int f) { return fmt_info(f).has_mins; }
constexpr bool has_sums(int f) { return fmt_info(f).has_sums; }
constexpr int code_offset(int f) { return fmt_info(f).code_offset; }
constexpr bool q8_1_only(int f) { return fmt_info(f).q8_1_only; }

// fn(ic<I>{}) for i == I in 0..MAX, which instantiates fn for exactly those; hipErrorInvalidValue
// for any other i
template <int V> using ic = std::integral_constant<int, V>;
template <int MAX, int I = 0, class Fn> hipError_t dispatch_upto(int i, Fn &&fn)
{
    if constexpr (I <= MAX) {
        if (i == I) return fn(ic<I>{});
        return dispatch_upto<MAX, I + 1>(i, fn);
    } else {
        return hipErrorInvalidValue;
    }
}
// fn(ic<F>{}) for the table's type fmt; hipErrorInvalidValue for an unknown one
template <class Fn> hipError_t dispatch_fmt(int fmt, Fn &&fn) { return dispatch_upto<kNumFmts - 1>(fmt, fn); }
// fn(ic<NB>{}) for a token-tile count nb in {1, 2, 4, 8} (pick_nb's values: tiles of 16*nb tokens);
// hipErrorInvalidValue for any other
template <class Fn> hipError_t dispatch_nb(int nb, Fn &&fn)
{
    switch (nb) {
    case 1: return fn(ic<1>{});
    case 2: return fn(ic<2>{});
    case 4: return fn(ic<4>{});
    case 8: return fn(ic<8>{});
    default: return hipErrorInvalidValue;
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 ld16(const void *p)
{
#ifdef GQ_ALIGN_TEST // diagnostic only: same access pattern with 16-byte aligned addresses
    p = (const void *)((uintptr_t)p & ~(uintptr_t)15);
#endif
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

__device__ __forceinline__ u32x2 ld8(const void *p)
{
#ifdef GQ_ALIGN_TEST
    p = (const void *)((uintptr_t)p & ~(uintptr_t)7);
#endif
    u32x2 v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

__device__ __forceinline__ uint32_t ld4(const void *p)
{
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

__device__ __forceinline__ uint16_t ld2(const void *p)
{
    uint16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

__device__ __forceinline__ float h2f(uint32_t bits16)
{
    return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16);
}

__device__ __forceinline__ uint16_t f2h_bits(float f)
{
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}

// v = four consecutive output rows (row..row + 3 of M) of one token, dst = the first one's fp16:
// one packed 8-byte store (2-byte aligned when ldc or M is odd: an unaligned store), or the rows
// below M one by one in the last, partial group.  Four epilogues keep this text in place (gemm_kernel,
// store_c_tiles, ilc_sum, reduce_grouped_kernel): called through the function they compile to other
// machine code -- the tail's compares hoisted or rescheduled ("The 256-row tile family")
template <class R, class L> __device__ __forceinline__ void store_h4(uint16_t *dst, const f32x4 v, R row, L M)
{
    if (row + 4 <= M) {
        *(u32x2 *)dst = (u32x2){(uint32_t)f2h_bits(v[0]) | ((uint32_t)f2h_bits(v[1]) << 16),
                                (uint32_t)f2h_bits(v[2]) | ((uint32_t)f2h_bits(v[3]) << 16)};
    } else {
        for (int i = 0; i < 4 && row + i < M; ++i) dst[i] = f2h_bits(v[i]);
    }
}

// v_dot4_i32_i8: c + sum_k a.i8[k] * b.i8[k]
__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

__device__ __forceinline__ uint32_t byte_of(uint32_t w, uint32_t k) { return (w >> (8 * k)) & 0xffu; }

// Q4_K 6-bit scale and min of sub-block j from the 12 scale bytes s0..s11 packed in
// words sw[0..2] (== get_scale_min_k4; kernels/mmq_q4_k.py:30-80).
__device__ __forceinline__ void q4k_sc_m(const uint32_t sw[3], int j, int &sc, int &m)
{
    if (j < 4) {
        sc = byte_of(sw[0], j) & 63;
        m = byte_of(sw[1], j) & 63;
    } else {
        uint32_t hi = byte_of(sw[2], j - 4);
        sc = (hi & 0x0f) | ((byte_of(sw[0], j - 4) >> 6) << 4);
        m = (hi >> 4) | ((byte_of(sw[1], j - 4) >> 6) << 4);
    }
}

// s_waitcnt vmcnt(n) for a wave-uniform n <= MAXN (the immediate is an encoding field): the
// steady-state count is the first compare, the pipeline tails walk down from it
template <int MAXN> __device__ __attribute__((always_inline)) inline void vm_wait(int n)
{
    if constexpr (MAXN <= 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
        if (n >= MAXN) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(MAXN) : "memory");
        else vm_wait<MAXN - 1>(n);
    }
}

} // namespace gq

// rmsnorm.hip -- residual add + RMSNorm, optionally straight into a gq_mmq workspace's activation
// part (gq_rmsnorm / gq_rmsnorm_prepare; no reference counterpart).
//
// One workgroup of 256 lanes per token row.  Lane t owns the 8 consecutive fp16 k = 2048 c + 8 t ..
// + 7 of every 2048-element chunk c (one 16-byte load), so an aligned group of 4 lanes owns a q8_1
// block and gguf_q8_1.hpp's q8_1_quad / deq_words apply to the normed row as they do to act_quant's
// input.  Per row:
//   h[k]  = R ? fp16(float(x[k]) + float(r[k])) : x[k]         (one rounding: fp32 holds the sum)
//   ss    = sum_k float(h[k])^2 in fp32: every lane adds its own squares in k order (each square
//           is exact in fp32, lanes and chunks past K add zeros), the 64 lanes of a wave meet in a
//           6-step xor butterfly, the four waves through 16 bytes of LDS as (w0 + w1) + (w2 + w3).
//           The order is a function of K alone: not of N, the row, a stride, a base or the outputs.
//   scale = 1 / sqrtf(ss / K + eps)                            (IEEE division and square root)
//   y[k]  = fp16((float(h[k]) * scale) * w[k])                 (two fp32 products, one fp16 rounding)
// Rows up to kNormRegChunks chunks (K <= 16384) stay in registers between the two passes; a longer
// row is read again -- from H where the call stores it (H may BE X or R: then the first pass has
// overwritten them), else x and r once more and the same sum.
// Outputs, each optional: H, Y, and the forms act_quant writes for q8_1 at this (N, K): SOA codes +
// d + s (+ the fp16 copy xraw = y) at decode token counts, else the DEQ x~ in its (0,2,1,3) order.
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_q8_1.hpp"

namespace gq {

__device__ __forceinline__ void st16(void *p, u32x4 v) { __builtin_memcpy(p, &v, 16); }

// the lane's 8 values of h at x / r (r may be null)
__device__ __forceinline__ u32x4 norm_h(const uint16_t *x, const uint16_t *r)
{
    const u32x4 a = ld16(x);
    if (!r) return a;
    const u32x4 b = ld16(r);
    u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = h2f(a[i] & 0xffff) + h2f(b[i] & 0xffff), hi = h2f(a[i] >> 16) + h2f(b[i] >> 16);
        o[i] = (uint32_t)f2h_bits(lo) | ((uint32_t)f2h_bits(hi) << 16);
    }
    return o;
}

__device__ __forceinline__ float norm_sumsq(u32x4 h, float acc)
{
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo = h2f(h[i] & 0xffff), hi = h2f(h[i] >> 16);
        acc = __builtin_fmaf(lo, lo, acc); // (the square is exact: the fma is the sum's one rounding)
        acc = __builtin_fmaf(hi, hi, acc);
    }
    return acc;
}

// NCH > 0: the row's NCH chunks in registers.  NCH == 0: any K, the row read twice.
template <int NCH>
__global__ __launch_bounds__(256) void rmsnorm_kernel(const NormArgs a)
{
    __shared__ float part[4];
    const int64_t row = (int64_t)blockIdx.x, K = a.K;
    const int t = threadIdx.x;
    const uint16_t *x = a.X + row * a.ldx;
    const uint16_t *r = a.R ? a.R + row * a.ldr : nullptr;
    uint16_t *hrow = a.H ? a.H + row * a.ldh : nullptr;

    float ss = 0.f;
    u32x4 hreg[NCH > 0 ? NCH : 1];
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int64_t k = (int64_t)c * kNormChunk + 8 * t;
            hreg[c] = (u32x4){0, 0, 0, 0};
            if (k < K) {
                hreg[c] = norm_h(x + k, r ? r + k : nullptr);
                if (hrow) st16(hrow + k, hreg[c]);
            }
            ss = norm_sumsq(hreg[c], ss);
        }
    } else {
        for (int64_t k0 = 0; k0 < K; k0 += kNormChunk) {
            const int64_t k = k0 + 8 * t;
            u32x4 h = {0, 0, 0, 0};
            if (k < K) {
                h = norm_h(x + k, r ? r + k : nullptr);
                if (hrow) st16(hrow + k, h);
            }
            ss = norm_sumsq(h, ss);
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
    if ((t & 63) == 0) part[t >> 6] = ss;
    __syncthreads();
    ss = (part[0] + part[1]) + (part[2] + part[3]);
    const float scale = 1.0f / sqrtf(ss / (float)K + a.eps);

    uint16_t *yrow = a.Y ? a.Y + row * a.ldy : nullptr;
    const int64_t nb = K / 32;
    const bool quant = a.xq || a.xdeq;
    auto second = [&](const u32x4 h, const int64_t k, const bool live) {
        u32x4 y = {0, 0, 0, 0};
        if (live) {
            float w[8];
            __builtin_memcpy(w, a.w + k, 32);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float lo = (h2f(h[i] & 0xffff) * scale) * w[2 * i], hi = (h2f(h[i] >> 16) * scale) * w[2 * i + 1];
                y[i] = (uint32_t)f2h_bits(lo) | ((uint32_t)f2h_bits(hi) << 16);
            }
            if (yrow) st16(yrow + k, y);
            if (a.xraw) st16(a.xraw + row * K + k, y);
        }
        if (!quant) return;
        const Q81Quad q = q8_1_quad(y); // (every lane: DPP quad groups; a quad is live or dead as one)
        if (!live) return;
        if (a.xdeq) {
            st16(a.xdeq + row * K + k, deq_words(q));
        } else {
            *(u32x2 *)(a.xq + row * K + k) = (u32x2){q.codes[0], q.codes[1]};
            if ((t & 3) == 0) {
                a.xd[row * nb + (k >> 5)] = q.d;
                a.xs[row * nb + (k >> 5)] = h2f(q.sbits);
            }
        }
    };
    if constexpr (NCH > 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            const int64_t k = (int64_t)c * kNormChunk + 8 * t;
            second(hreg[c], k, k < K);
        }
    } else {
        for (int64_t k0 = 0; k0 < K; k0 += kNormChunk) {
            const int64_t k = k0 + 8 * t;
            const bool live = k < K;
            u32x4 h = {0, 0, 0, 0};
            if (live) h = hrow ? ld16(hrow + k) : norm_h(x + k, r ? r + k : nullptr);
            second(h, k, live);
        }
    }
}

hipError_t launch_rmsnorm(const NormArgs &a, int64_t N, hipStream_t s)
{
    if (N == 0 || a.K == 0) return hipSuccess;
    if (N > INT32_MAX || a.K % 32 != 0) return hipErrorInvalidValue;
    const dim3 grid((unsigned)N), block(256);
    const int64_t nch = (a.K + kNormChunk - 1) / kNormChunk;
    if (nch <= 1) rmsnorm_kernel<1><<<grid, block, 0, s>>>(a);
    else if (nch <= 2) rmsnorm_kernel<2><<<grid, block, 0, s>>>(a);
    else if (nch <= 4) rmsnorm_kernel<4><<<grid, block, 0, s>>>(a);
    else if (nch <= kNormRegChunks) rmsnorm_kernel<kNormRegChunks><<<grid, block, 0, s>>>(a);
    else rmsnorm_kernel<0><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

} // namespace gq

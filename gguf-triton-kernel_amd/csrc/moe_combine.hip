// moe_combine.hip -- the router-weighted sum over slots that ends a mixture-of-experts FFN block
// (gq_moe_combine): Y[n][m] = fp16(sum_s W[n][s] * D[n][s][m]).
//
// A memory-bound elementwise kernel: every thread owns 8 consecutive outputs of one token (one
// 16-byte load per slot, one 16-byte store when the rows are 16-byte aligned; element by element
// otherwise and in a row's last partial chunk) and walks the S slots in order.  The arithmetic is
// fixed so that the result is a function of the inputs alone: acc = 0, then for s = 0..S-1
// acc = acc + w * d as two fp32 operations -- no fused multiply-add, no reassociation, no atomics
// -- and one round-to-nearest-even to fp16 at the end.
// gq_moe_combine_shared adds a shared expert's term after the slots, in a kernel of its own:
// acc = acc + dsh, or acc = acc + gate[n] * dsh with a per-token fp32 gate.
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"

// the defined arithmetic is an fp32 multiply, then an fp32 add: the compiler's default would fuse
// them into one fma (with fp32 weights the product is not exact, so the bits would differ)
#pragma clang fp contract(off)

namespace gq {

namespace {

constexpr int CB_THREADS = 256, CB_VEC = 8;

// (written here, under the pragma: the toolkit's __fmul_rn / __fadd_rn are a plain * and + that the
// compiler contracts like any other)
__device__ __forceinline__ float mul32(float a, float b) { return a * b; }
__device__ __forceinline__ float add32(float a, float b) { return a + b; }

template <bool WF32> __device__ __forceinline__ float combine_w(const void *W, int64_t i)
{
    if constexpr (WF32) return ((const float *)W)[i];
    return h2f(((const uint16_t *)W)[i]);
}

// VEC: D, Y 16-byte aligned and ldd, ldy multiples of 8 (every whole chunk is an aligned 16 bytes)
template <bool WF32, bool VEC>
__global__ __launch_bounds__(CB_THREADS) void moe_combine_kernel(const uint16_t *__restrict__ D, const void *__restrict__ W,
                                                                 uint16_t *__restrict__ Y, int64_t N, int S, int64_t M,
                                                                 int64_t ldd, int64_t ldy, int64_t chunks)
{
    const int64_t total = N * chunks, step = (int64_t)gridDim.x * CB_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x; i < total; i += step) {
        const int64_t n = i / chunks, m0 = (i - n * chunks) * CB_VEC;
        const int cnt = M - m0 < CB_VEC ? (int)(M - m0) : CB_VEC;
        float acc[CB_VEC];
#pragma unroll
        for (int k = 0; k < CB_VEC; ++k) acc[k] = 0.f;
        if (VEC && cnt == CB_VEC) {
            for (int s = 0; s < S; ++s) {
                const float w = combine_w<WF32>(W, n * S + s);
                const u32x4 d = *(const u32x4 *)(D + (n * S + s) * ldd + m0);
                const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int k = 0; k < CB_VEC; ++k)
                    acc[k] = add32(acc[k], mul32(w, h2f((dw[k >> 1] >> (16 * (k & 1))) & 0xffffu)));
            }
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (uint32_t)f2h_bits(acc[2 * k]) | ((uint32_t)f2h_bits(acc[2 * k + 1]) << 16);
            *(u32x4 *)(Y + n * ldy + m0) = (u32x4){o[0], o[1], o[2], o[3]};
        } else {
            for (int s = 0; s < S; ++s) {
                const float w = combine_w<WF32>(W, n * S + s);
                const uint16_t *d = D + (n * S + s) * ldd + m0;
#pragma unroll
                for (int k = 0; k < CB_VEC; ++k)
                    if (k < cnt) acc[k] = add32(acc[k], mul32(w, h2f(d[k])));
            }
#pragma unroll
            for (int k = 0; k < CB_VEC; ++k)
                if (k < cnt) Y[n * ldy + m0 + k] = f2h_bits(acc[k]);
        }
    }
}

// gq_moe_combine_shared: the slot sum above, then the shared expert's term -- acc = acc + dsh, or
// with GATE acc = acc + gate[n] * dsh (two fp32 operations again).  A kernel of its own:
// moe_combine_kernel stays the code it is.  VEC: Dsh and ldsh aligned as D and ldd.
template <bool WF32, bool VEC, bool GATE>
__global__ __launch_bounds__(CB_THREADS) void moe_combine_shared_kernel(const uint16_t *__restrict__ D,
                                                                        const void *__restrict__ W,
                                                                        const uint16_t *__restrict__ Dsh,
                                                                        const float *__restrict__ gate,
                                                                        uint16_t *__restrict__ Y, int64_t N, int S, int64_t M,
                                                                        int64_t ldd, int64_t ldsh, int64_t ldy, int64_t chunks)
{
    const int64_t total = N * chunks, step = (int64_t)gridDim.x * CB_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CB_THREADS + threadIdx.x; i < total; i += step) {
        const int64_t n = i / chunks, m0 = (i - n * chunks) * CB_VEC;
        const int cnt = M - m0 < CB_VEC ? (int)(M - m0) : CB_VEC;
        float gn = 1.f;
        if constexpr (GATE) gn = gate[n];
        auto shared = [&](float dsh) { return GATE ? mul32(gn, dsh) : dsh; };
        float acc[CB_VEC];
#pragma unroll
        for (int k = 0; k < CB_VEC; ++k) acc[k] = 0.f;
        if (VEC && cnt == CB_VEC) {
            for (int s = 0; s < S; ++s) {
                const float w = combine_w<WF32>(W, n * S + s);
                const u32x4 d = *(const u32x4 *)(D + (n * S + s) * ldd + m0);
                const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
                for (int k = 0; k < CB_VEC; ++k)
                    acc[k] = add32(acc[k], mul32(w, h2f((dw[k >> 1] >> (16 * (k & 1))) & 0xffffu)));
            }
            const u32x4 d = *(const u32x4 *)(Dsh + n * ldsh + m0);
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < CB_VEC; ++k) acc[k] = add32(acc[k], shared(h2f((dw[k >> 1] >> (16 * (k & 1))) & 0xffffu)));
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = (uint32_t)f2h_bits(acc[2 * k]) | ((uint32_t)f2h_bits(acc[2 * k + 1]) << 16);
            *(u32x4 *)(Y + n * ldy + m0) = (u32x4){o[0], o[1], o[2], o[3]};
        } else {
            for (int s = 0; s < S; ++s) {
                const float w = combine_w<WF32>(W, n * S + s);
                const uint16_t *d = D + (n * S + s) * ldd + m0;
#pragma unroll
                for (int k = 0; k < CB_VEC; ++k)
                    if (k < cnt) acc[k] = add32(acc[k], mul32(w, h2f(d[k])));
            }
            const uint16_t *d = Dsh + n * ldsh + m0;
#pragma unroll
            for (int k = 0; k < CB_VEC; ++k)
                if (k < cnt) Y[n * ldy + m0 + k] = f2h_bits(add32(acc[k], shared(h2f(d[k]))));
        }
    }
}

} // namespace

hipError_t launch_moe_combine_shared(const uint16_t *D, const void *W, bool w_f32, const uint16_t *Dsh, int64_t ldsh,
                                     const float *gate, uint16_t *Y, int64_t N, int64_t S, int64_t M, int64_t ldd,
                                     int64_t ldy, hipStream_t s)
{
    if (N < 1 || S < 1 || M < 1) return hipErrorInvalidValue;
    const int64_t chunks = (M + CB_VEC - 1) / CB_VEC;
    if (N > INT64_MAX / chunks) return hipErrorInvalidValue;
    const int64_t blocks = (N * chunks + CB_THREADS - 1) / CB_THREADS;
    const int64_t cap = (int64_t)num_cus() * 32; // grid-stride beyond a few rounds of the chip
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    const bool vec = (((uintptr_t)D | (uintptr_t)Dsh | (uintptr_t)Y) & 15) == 0 && ldd % CB_VEC == 0 &&
                     ldsh % CB_VEC == 0 && ldy % CB_VEC == 0;
    auto go = [&](auto wf, auto v, auto g) {
        moe_combine_shared_kernel<decltype(wf)::value != 0, decltype(v)::value != 0, decltype(g)::value != 0>
            <<<dim3(grid), dim3(CB_THREADS), 0, s>>>(D, W, Dsh, gate, Y, N, (int)S, M, ldd, ldsh, ldy, chunks);
        return hipGetLastError();
    };
    auto by_gate = [&](auto wf, auto v) { return gate ? go(wf, v, ic<1>{}) : go(wf, v, ic<0>{}); };
    if (w_f32) return vec ? by_gate(ic<1>{}, ic<1>{}) : by_gate(ic<1>{}, ic<0>{});
    return vec ? by_gate(ic<0>{}, ic<1>{}) : by_gate(ic<0>{}, ic<0>{});
}

hipError_t launch_moe_combine(const uint16_t *D, const void *W, bool w_f32, uint16_t *Y, int64_t N, int64_t S, int64_t M,
                              int64_t ldd, int64_t ldy, hipStream_t s)
{
    if (N < 1 || S < 1 || M < 1) return hipErrorInvalidValue;
    const int64_t chunks = (M + CB_VEC - 1) / CB_VEC;
    if (N > INT64_MAX / chunks) return hipErrorInvalidValue;
    const int64_t blocks = (N * chunks + CB_THREADS - 1) / CB_THREADS;
    const int64_t cap = (int64_t)num_cus() * 32; // grid-stride beyond a few rounds of the chip
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    const bool vec = (((uintptr_t)D | (uintptr_t)Y) & 15) == 0 && ldd % CB_VEC == 0 && ldy % CB_VEC == 0;
    auto go = [&](auto wf, auto v) {
        moe_combine_kernel<decltype(wf)::value != 0, decltype(v)::value != 0>
            <<<dim3(grid), dim3(CB_THREADS), 0, s>>>(D, W, Y, N, (int)S, M, ldd, ldy, chunks);
        return hipGetLastError();
    };
    if (w_f32) return vec ? go(ic<1>{}, ic<1>{}) : go(ic<1>{}, ic<0>{});
    return vec ? go(ic<0>{}, ic<1>{}) : go(ic<0>{}, ic<0>{});
}

} // namespace gq

// moe_route.hip -- the router of a mixture-of-experts block on the device (gq_moe_route,
// gq_moe_topk): from a token's hidden state to its S expert ids and their weights.
//
// Two kernels, both without atomics and with a fixed arithmetic order, so that a token's result is
// a function of its own row alone:
//
// moe_logits_kernel: L[n][e] = sum_k X[n][k] * Wr[e][k] in fp32.  One workgroup per expert row, so
//   the router matrix is streamed once per tile of RT tokens and never once per token; the four
//   waves take the row's 256-element chunks round robin, every lane four consecutive k of a chunk.
//   A (token, expert) sum is: per lane acc = fmaf(x, w, acc) over its k ascending; a 64-lane xor
//   butterfly (offsets 32 .. 1); the four waves' sums added in wave order by one thread.  Nothing in
//   that order depends on N or on the token's place in its tile.  Weights and activations go
//   straight to registers: no wave shares another's k range, so an LDS copy would serve nobody.
//
// moe_topk_kernel: one wave per token.  Expert e = 64*j + lane sits in lane's register j as a 64-bit
//   word (order-preserving image of the fp32 key << 32 | 1024 - e), so an unsigned maximum is "largest
//   key, lowest index on ties", a NaN key (image 0) ranks below -inf, and a taken or absent expert
//   (word 0) below everything: S rounds of a register maximum and a wave butterfly always find S
//   distinct experts.  Lane s then owns slot s: its value, the sum over the slots, one store each.
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"

namespace gq {

namespace {

constexpr int RT_THREADS = 256, RT_WAVES = 4, RT_CHUNK = 256; // a wave's chunk: 64 lanes x 4 elements
constexpr int TK_THREADS = 256, TK_WAVES = 4;

__device__ __forceinline__ float wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// RT: tokens per pass over the row (1, 2, 4 or 8; rows past N - 1 re-read row N - 1 and are not
// stored).  WH: the router matrix is fp16.
template <bool WH, int RT>
__global__ __launch_bounds__(RT_THREADS) void moe_logits_kernel(const void *__restrict__ Wr, const uint16_t *__restrict__ X,
                                                                int64_t ldx, float *__restrict__ L, int64_t ldl, int N, int H)
{
    __shared__ float red[RT_WAVES][RT];
    const int e = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint8_t *wrow = (const uint8_t *)Wr + (int64_t)e * H * (WH ? 2 : 4);
    for (int n0 = 0; n0 < N; n0 += RT) {
        float acc[RT];
        const uint16_t *xrow[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            acc[t] = 0.f;
            xrow[t] = X + (int64_t)(n0 + t < N ? n0 + t : N - 1) * ldx;
        }
#pragma unroll 2
        for (int k = wave * RT_CHUNK + lane * 4; k < H; k += RT_WAVES * RT_CHUNK) {
            float w[4];
            if constexpr (WH) {
                const u32x2 v = ld8(wrow + (int64_t)k * 2);
                w[0] = h2f(v.x & 0xffffu), w[1] = h2f(v.x >> 16), w[2] = h2f(v.y & 0xffffu), w[3] = h2f(v.y >> 16);
            } else {
                __builtin_memcpy(w, wrow + (int64_t)k * 4, 16); // (one 16-byte load at any alignment)
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const u32x2 x = ld8(xrow[t] + k);
                acc[t] = fmaf(h2f(x.x & 0xffffu), w[0], acc[t]);
                acc[t] = fmaf(h2f(x.x >> 16), w[1], acc[t]);
                acc[t] = fmaf(h2f(x.y & 0xffffu), w[2], acc[t]);
                acc[t] = fmaf(h2f(x.y >> 16), w[3], acc[t]);
            }
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const float s = wave_sum(acc[t]);
            if (lane == 0) red[wave][t] = s;
        }
        __syncthreads();
        if (threadIdx.x < RT && n0 + (int)threadIdx.x < N) {
            const int t = threadIdx.x;
            L[(int64_t)(n0 + t) * ldl + e] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
        }
        __syncthreads(); // (red is rewritten by the next pass)
    }
}

// Order-preserving image of an fp32 key: a < b  <=>  image(a) < image(b); -0 and +0 share one
// image; NaN -> 0, below -inf's 0x007fffff.
__device__ __forceinline__ uint32_t key_image(float k)
{
    uint32_t b = __builtin_bit_cast(uint32_t, k);
    const uint32_t a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return 0u;
    if (a == 0u) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float sigmoid32(float l) { return 1.f / (1.f + expf(-l)); }

// KPL: experts per lane, E <= 64 * KPL.  func 0 softmax, 1 sigmoid.
template <int KPL>
__global__ __launch_bounds__(TK_THREADS) void moe_topk_kernel(const float *__restrict__ logits, int64_t ldl,
                                                              const float *__restrict__ bias, int func, int norm, float scale,
                                                              int32_t *__restrict__ ids, void *__restrict__ W, int w_f32,
                                                              int64_t N, int E, int S)
{
    const int lane = threadIdx.x & 63;
    const int64_t step = (int64_t)gridDim.x * TK_WAVES;
    for (int64_t n = (int64_t)blockIdx.x * TK_WAVES + (threadIdx.x >> 6); n < N; n += step) { // (wave-uniform)
        const float *row = logits + n * ldl;
        uint64_t word[KPL];
        float l[KPL], mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int e = 64 * j + lane;
            l[j] = -INFINITY;
            word[j] = 0;
            if (e < E) {
                l[j] = row[e];
                const float key = (func == 1 && bias) ? sigmoid32(l[j]) + bias[e] : l[j];
                word[j] = ((uint64_t)key_image(key) << 32) | (uint32_t)(1024 - e);
            }
            mx = fmaxf(mx, l[j]);
        }
        int mine = 0;
        for (int s = 0; s < S; ++s) {
            uint64_t best = word[0];
#pragma unroll
            for (int j = 1; j < KPL; ++j) best = word[j] > best ? word[j] : best;
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) {
                const uint64_t o = __shfl_xor((unsigned long long)best, off);
                best = o > best ? o : best;
            }
            // (S <= E: an untaken expert's word is >= 1, so best names one; the clamp only keeps a
            // caller's broken S > E from ever writing an id outside [0, E))
            int e = 1024 - (int)(uint32_t)best;
            e = e < 0 ? 0 : (e >= E ? E - 1 : e);
#pragma unroll
            for (int j = 0; j < KPL; ++j)
                if (word[j] == best) word[j] = 0; // (words are unique: one lane's one register)
            if (lane == s) mine = e;
        }
        float v = 0.f, denom = 1.f;
        if (func == 0) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            if (lane < S) v = expf(row[mine] - mx);
            if (!norm) { // the softmax denominator over all E (absent experts: expf(-inf) = 0)
                float part = 0.f;
#pragma unroll
                for (int j = 0; j < KPL; ++j) part += expf(l[j] - mx);
                denom = wave_sum(part);
            }
        } else if (lane < S) {
            v = sigmoid32(row[mine]);
        }
        if (norm) denom = wave_sum(v); // (lanes past S hold 0; softmax: the all-E denominator cancels)
        const float w = v / denom * scale;
        if (lane < S) {
            ids[n * S + lane] = mine;
            if (w_f32)
                ((float *)W)[n * S + lane] = w;
            else
                ((uint16_t *)W)[n * S + lane] = f2h_bits(w);
        }
    }
}

} // namespace

bool moe_topk_ok(int64_t E, int64_t S) { return S >= 1 && S <= E && E <= kMaxSortExperts && S <= kMaxIdPairs; }

bool moe_logits_ok(int64_t N, int64_t H) { return N <= kMaxRouteTokens && H % 32 == 0 && H <= INT32_MAX; }

hipError_t launch_moe_logits(const void *Wr, bool wr_f16, const uint16_t *X, int64_t ldx, float *L, int64_t ldl, int64_t N,
                             int64_t E, int64_t H, hipStream_t s)
{
    if (N < 1 || E < 1 || E > kMaxSortExperts || !moe_logits_ok(N, H)) return hipErrorInvalidValue;
    auto go = [&](auto wh, auto rt) {
        moe_logits_kernel<decltype(wh)::value != 0, decltype(rt)::value>
            <<<dim3((unsigned)E), dim3(RT_THREADS), 0, s>>>(Wr, X, ldx, L, ldl, (int)N, (int)H);
        return hipGetLastError();
    };
    auto by_tile = [&](auto wh) {
        if (N == 1) return go(wh, ic<1>{});
        if (N == 2) return go(wh, ic<2>{});
        if (N <= 4) return go(wh, ic<4>{});
        return go(wh, ic<8>{});
    };
    return wr_f16 ? by_tile(ic<1>{}) : by_tile(ic<0>{});
}

hipError_t launch_moe_topk(const float *logits, int64_t ldl, const float *bias, int func, bool norm, float scale, int32_t *ids,
                           void *W, bool w_f32, int64_t N, int64_t E, int64_t S, hipStream_t s)
{
    if (N < 1 || !moe_topk_ok(E, S)) return hipErrorInvalidValue;
    const int64_t blocks = (N + TK_WAVES - 1) / TK_WAVES;
    const int64_t cap = (int64_t)num_cus() * 32; // grid-stride beyond a few rounds of the chip
    const unsigned grid = (unsigned)(blocks < cap ? blocks : cap);
    auto go = [&](auto kpl) {
        moe_topk_kernel<decltype(kpl)::value><<<dim3(grid), dim3(TK_THREADS), 0, s>>>(
            logits, ldl, bias, func, norm ? 1 : 0, scale, ids, W, w_f32 ? 1 : 0, N, (int)E, (int)S);
        return hipGetLastError();
    };
    if (E <= 64) return go(ic<1>{});
    if (E <= 128) return go(ic<2>{});
    if (E <= 256) return go(ic<4>{});
    if (E <= 512) return go(ic<8>{});
    return go(ic<16>{});
}

} // namespace gq

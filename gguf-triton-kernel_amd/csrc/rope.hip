// rope.hip -- the step between a block's q/k/v projections and its attention, in one launch
// (gq_rope_append): an optional per-head RMSNorm of q and k, the rotary position embedding of both,
// q to its output and k and v into the fp16 or Q8_0 KV cache.  No reference counterpart.
//
// Work split.  A token has J = n_head + 2 n_kv_head head jobs: its q heads, its k heads, its v heads.
// A head is D/2 lanes, lane l of it owning two elements, so a wave takes one head (D = 128) or two
// (D = 64, one per half-wave) at a time.  Workgroup (x, y) of 4 waves walks the tokens x, x + gridDim.x,
// ... and takes, of each, the y-th share of the head jobs: `passes` rounds of 4 waves x 128/D heads.
// The grid is fixed on the host from B * N, the head counts and the compute units: one token is spread
// over up to J D / 512 workgroups, thousands of tokens get one share each and a token loop.  No length
// enters it: the position p = kv_len[b] - N + i is read on the device.
//
// The angle.  Lane l < n_rot/2 owns rotation pair l in both modes, so its (m cos, m sin) is computed
// ONCE per token and kept in two registers over all the head jobs the wave loops over.  theta = p f
// is formed in fp64 (exact: 31 x 24 bits), reduced there by quarter turns to |r| <= pi/4 (two fmas
// against a two-word pi/2), and only r goes to fp32: a degree-7 / degree-8 minimax pair (the Cephes
// single-precision coefficients, evaluated with fmas, ~1 ulp) gives sin and cos and the quadrant swaps
// and negates them.  No v_sin_f32 / v_cos_f32, no fp32 product of a position and a frequency.
//
// Lanes and elements.  NORM mode: lane l owns elements (2l, 2l + 1), one 4-byte access where the
// pointers allow it.  NEOX mode with h = n_rot/2: lane l < h owns its pair (l, l + h), lane l >= h
// the pass-through elements (l + h, l + D/2) -- two coalesced 2-byte streams.  v heads use the NORM
// layout in either mode.  The norm's sum over D is an xor butterfly over the head's D/2 lanes.
//
// Q8_0.  A block's 32 elements are 16 lanes of the NORM layout: the amax is a 4-step xor butterfly,
// each lane writes its two codes as one 2-byte store and the block's first lane the scale (the 34-byte
// blocks are 2-byte aligned only).  A NEOX k head is first brought into the NORM layout by two
// ds_bpermute reads of the packed fp16 pair, so one quantizer serves every n_rot.  The arithmetic is
// qblk::q8_scale / q8_code, q8_block's own steps: gq_kv_append's bytes of the same fp16 values.
//
// D = 256 (Gemma; rope_append256_kernel).  A head is 128 lane jobs, so a wave takes one head with TWO
// jobs per lane: virtual lanes l and l + 64 of the layouts above (lane l owns rotation pairs l and
// l + 64 where they exist).  Everything per lane comes in twos -- the angle, the norm weights, the
// element indices -- the norm's sum adds the lane's two partial sums before the 64-lane butterfly, a
// Q8_0 block is still 16 consecutive lanes of one job, and the NEOX-to-NORM gather reads both jobs of
// the holding lane and picks one.  Same grid, same arithmetic, same bytes.
//
// No LDS, no scratch, no atomics, no wait between workgroups.  In place (Qout == Q) is safe: a lane
// writes the two elements it read.
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_rope.hpp"
#include "quant/gguf_quant_blocks.hpp"

namespace gq {
namespace {

struct RopeArgs {
    const uint16_t *Q, *Kn, *Vn;
    uint16_t *Qo;
    uint8_t *Kc, *Vc;
    const int32_t *kv_len;
    const float *inv_freq, *wq, *wk;
    int64_t ldq, ldk, ldv, ldqo, tok_stride, head_stride, seq_stride, T;
    int capacity, N, n_head, n_kv, n_rot, passes;
    float mscale, eps;
    bool rows4, cache4; // 4-byte accesses allowed: the q/k/v/Qout rows, the fp16 cache rows
};

template <int KV, int D, int MODE, bool HAS_NORM>
__global__ __launch_bounds__(256) void rope_append_kernel(const RopeArgs a)
{
    constexpr int HL = D / 2;   // lanes per head
    constexpr int HPW = 64 / HL; // heads per wave and pass
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & (HL - 1), half = lane / HL;
    const int h = a.n_rot >> 1, J = a.n_head + 2 * a.n_kv;
    const bool rot = li < h;
    // this lane's elements of a q or k head
    int r0 = 2 * li, r1 = 2 * li + 1;
    if (MODE == 1) r0 = rot ? li : li + h, r1 = rot ? li + h : li + HL;
    // NEOX: the lanes of this head that hold elements 2 li and 2 li + 1, and the slot there
    int from0 = lane, from1 = lane, slot0 = 0, slot1 = 1;
    if (MODE == 1 && KV == 1) {
        auto holder = [&](int e, int &ln, int &slot) {
            if (e < 2 * h) ln = e < h ? e : e - h, slot = e >= h;
            else ln = e < HL + h ? e - h : e - HL, slot = e >= HL + h;
            ln += half * HL;
        };
        holder(2 * li, from0, slot0);
        holder(2 * li + 1, from1, slot1);
    }
    const float f = rot ? a.inv_freq[li] : 0.f;
    float wq0 = 1.f, wq1 = 1.f, wk0 = 1.f, wk1 = 1.f;
    if (HAS_NORM) wq0 = a.wq[r0], wq1 = a.wq[r1], wk0 = a.wk[r0], wk1 = a.wk[r1];

    for (int64_t t = blockIdx.x; t < a.T; t += gridDim.x) {
        const int b = (int)(t / a.N), i = (int)(t - (int64_t)b * a.N);
        const int p = a.kv_len[b] - a.N + i;
        const bool inside = p >= 0 && p < a.capacity; // (outside: the caller's error, no cache row written)
        float c, s;
        rope_cs(p, f, a.mscale, c, s);
        const int64_t crow = (int64_t)b * a.seq_stride + (int64_t)p * a.tok_stride;
        for (int k = 0; k < a.passes; ++k) {
            // (uniform over a head's lanes, as is every branch below: the shuffles stay inside a head)
            const int j = (((int)blockIdx.y * a.passes + k) * 4 + wave) * HPW + half;
            if (j >= J) continue;
            const bool isq = j < a.n_head, isv = j >= a.n_head + a.n_kv;
            const int hd = isq ? j : (isv ? j - a.n_head - a.n_kv : j - a.n_head);
            const uint16_t *src = (isq ? a.Q + t * a.ldq : (isv ? a.Vn + t * a.ldv : a.Kn + t * a.ldk)) + (int64_t)hd * D;
            const int e0 = isv ? 2 * li : r0, e1 = isv ? 2 * li + 1 : r1;
            const bool adj = MODE == 0 || isv;
            uint32_t o = load2(src, e0, e1, adj && a.rows4);
            if (!isv) {
                float y0 = h2f(o & 0xffff), y1 = h2f(o >> 16);
                if (HAS_NORM) {
                    float ss = __builtin_fmaf(y1, y1, y0 * y0);
#pragma unroll
                    for (int m = 1; m < HL; m <<= 1) ss += __shfl_xor(ss, m, 64);
                    const float scale = 1.0f / sqrtf(ss * (1.0f / D) + a.eps);
                    y0 = (y0 * scale) * (isq ? wq0 : wk0);
                    y1 = (y1 * scale) * (isq ? wq1 : wk1);
                }
                const float o0 = rot ? y0 * c - y1 * s : y0, o1 = rot ? y0 * s + y1 * c : y1;
                o = (uint32_t)f2h_bits(o0) | ((uint32_t)f2h_bits(o1) << 16);
            }
            if (isq) {
                store2(a.Qo + t * a.ldqo + (int64_t)hd * D, e0, e1, adj && a.rows4, o);
                continue;
            }
            uint8_t *dst = (isv ? a.Vc : a.Kc) + crow + (int64_t)hd * a.head_stride;
            if (KV == 0) {
                if (inside) store2((uint16_t *)dst, e0, e1, adj && a.cache4, o);
                continue;
            }
            if (MODE == 1 && !isv) { // into the NORM layout: elements (2 li, 2 li + 1)
                const uint32_t g0 = __shfl(o, from0, 64), g1 = __shfl(o, from1, 64);
                o = ((slot0 ? g0 >> 16 : g0) & 0xffff) | ((slot1 ? g1 >> 16 : g1 & 0xffff) << 16);
            }
            const uint16_t x0 = (uint16_t)o, x1 = (uint16_t)(o >> 16);
            float amax = fmaxf(fabsf(h2f((uint32_t)x0)), fabsf(h2f((uint32_t)x1))); // (fmaxf drops a NaN, as q8_block's max does)
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
            const uint16_t d = qblk::q8_scale<false>(amax);
            const float div = gq::h2f(d);
            const uint32_t codes = (uint32_t)(uint8_t)qblk::q8_code(x0, div) | ((uint32_t)(uint8_t)qblk::q8_code(x1, div) << 8);
            if (inside) {
                uint16_t *blk = (uint16_t *)(dst + 34 * (li >> 4));
                if ((li & 15) == 0) blk[0] = d;
                blk[1 + (li & 15)] = (uint16_t)codes;
            }
        }
    }
}

// D = 256: one wave per head, two jobs (virtual lanes lane and lane + 64) per lane -- the file header has the layout
template <int KV, int MODE, bool HAS_NORM>
__global__ __launch_bounds__(256) void rope_append256_kernel(const RopeArgs a)
{
    constexpr int D = 256, HL = 128;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = a.n_rot >> 1, J = a.n_head + 2 * a.n_kv;
    int li[2], r0[2], r1[2], from0[2], from1[2], slot0[2], slot1[2];
    bool rot[2];
    float f[2], wq0[2], wq1[2], wk0[2], wk1[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        li[s] = lane + 64 * s, rot[s] = li[s] < h;
        r0[s] = 2 * li[s], r1[s] = 2 * li[s] + 1;
        if (MODE == 1) r0[s] = rot[s] ? li[s] : li[s] + h, r1[s] = rot[s] ? li[s] + h : li[s] + HL;
        // NEOX: the virtual lanes that hold elements 2 li and 2 li + 1, and the half of their pair
        from0[s] = from1[s] = li[s], slot0[s] = 0, slot1[s] = 1;
        if (MODE == 1 && KV == 1) {
            auto holder = [&](int e, int &ln, int &slot) {
                if (e < 2 * h) ln = e < h ? e : e - h, slot = e >= h;
                else ln = e < HL + h ? e - h : e - HL, slot = e >= HL + h;
            };
            holder(2 * li[s], from0[s], slot0[s]);
            holder(2 * li[s] + 1, from1[s], slot1[s]);
        }
        f[s] = rot[s] ? a.inv_freq[li[s]] : 0.f;
        wq0[s] = wq1[s] = wk0[s] = wk1[s] = 1.f;
        if (HAS_NORM) wq0[s] = a.wq[r0[s]], wq1[s] = a.wq[r1[s]], wk0[s] = a.wk[r0[s]], wk1[s] = a.wk[r1[s]];
    }

    for (int64_t t = blockIdx.x; t < a.T; t += gridDim.x) {
        const int b = (int)(t / a.N), i = (int)(t - (int64_t)b * a.N);
        const int p = a.kv_len[b] - a.N + i;
        const bool inside = p >= 0 && p < a.capacity; // (outside: the caller's error, no cache row written)
        float c[2], sn[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) rope_cs(p, f[s], a.mscale, c[s], sn[s]);
        const int64_t crow = (int64_t)b * a.seq_stride + (int64_t)p * a.tok_stride;
        for (int k = 0; k < a.passes; ++k) {
            const int j = ((int)blockIdx.y * a.passes + k) * 4 + wave; // (wave-uniform, as is every branch below)
            if (j >= J) continue;
            const bool isq = j < a.n_head, isv = j >= a.n_head + a.n_kv;
            const int hd = isq ? j : (isv ? j - a.n_head - a.n_kv : j - a.n_head);
            const uint16_t *src = (isq ? a.Q + t * a.ldq : (isv ? a.Vn + t * a.ldv : a.Kn + t * a.ldk)) + (int64_t)hd * D;
            const bool adj = MODE == 0 || isv;
            int e0[2], e1[2];
            uint32_t o[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                e0[s] = isv ? 2 * li[s] : r0[s], e1[s] = isv ? 2 * li[s] + 1 : r1[s];
                o[s] = load2(src, e0[s], e1[s], adj && a.rows4);
            }
            if (!isv) {
                float y0[2], y1[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) y0[s] = h2f(o[s] & 0xffff), y1[s] = h2f(o[s] >> 16);
                if (HAS_NORM) {
                    float ss = __builtin_fmaf(y1[0], y1[0], y0[0] * y0[0]) + __builtin_fmaf(y1[1], y1[1], y0[1] * y0[1]);
#pragma unroll
                    for (int m = 1; m < 64; m <<= 1) ss += __shfl_xor(ss, m, 64);
                    const float scale = 1.0f / sqrtf(ss * (1.0f / D) + a.eps);
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        y0[s] = (y0[s] * scale) * (isq ? wq0[s] : wk0[s]);
                        y1[s] = (y1[s] * scale) * (isq ? wq1[s] : wk1[s]);
                    }
                }
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const float o0 = rot[s] ? y0[s] * c[s] - y1[s] * sn[s] : y0[s], o1 = rot[s] ? y0[s] * sn[s] + y1[s] * c[s] : y1[s];
                    o[s] = (uint32_t)f2h_bits(o0) | ((uint32_t)f2h_bits(o1) << 16);
                }
            }
            if (isq) {
#pragma unroll
                for (int s = 0; s < 2; ++s) store2(a.Qo + t * a.ldqo + (int64_t)hd * D, e0[s], e1[s], adj && a.rows4, o[s]);
                continue;
            }
            uint8_t *dst = (isv ? a.Vc : a.Kc) + crow + (int64_t)hd * a.head_stride;
            if (KV == 0) {
                if (inside) {
#pragma unroll
                    for (int s = 0; s < 2; ++s) store2((uint16_t *)dst, e0[s], e1[s], adj && a.cache4, o[s]);
                }
                continue;
            }
            if (MODE == 1 && !isv) { // into the NORM layout: job s gets elements (2 li, 2 li + 1) from the jobs that hold them
                uint32_t n[2];
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint32_t a0 = __shfl(o[0], from0[s] & 63, 64), a1 = __shfl(o[1], from0[s] & 63, 64);
                    const uint32_t b0 = __shfl(o[0], from1[s] & 63, 64), b1 = __shfl(o[1], from1[s] & 63, 64);
                    const uint32_t g0 = from0[s] >> 6 ? a1 : a0, g1 = from1[s] >> 6 ? b1 : b0;
                    n[s] = ((slot0[s] ? g0 >> 16 : g0) & 0xffff) | ((slot1[s] ? g1 >> 16 : g1 & 0xffff) << 16);
                }
                o[0] = n[0], o[1] = n[1];
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const uint16_t x0 = (uint16_t)o[s], x1 = (uint16_t)(o[s] >> 16);
                float amax = fmaxf(fabsf(h2f((uint32_t)x0)), fabsf(h2f((uint32_t)x1))); // (fmaxf drops a NaN, as q8_block's max does)
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
                const uint16_t d = qblk::q8_scale<false>(amax);
                const float div = gq::h2f(d);
                const uint32_t codes = (uint32_t)(uint8_t)qblk::q8_code(x0, div) | ((uint32_t)(uint8_t)qblk::q8_code(x1, div) << 8);
                if (inside) {
                    uint16_t *blk = (uint16_t *)(dst + 34 * (li[s] >> 4));
                    if ((li[s] & 15) == 0) blk[0] = d;
                    blk[1 + (li[s] & 15)] = (uint16_t)codes;
                }
            }
        }
    }
}

} // namespace

hipError_t launch_rope_append(int kv, int mode, const RopeCall &c, hipStream_t s)
{
    RopeArgs a{};
    a.Q = (const uint16_t *)c.Q, a.Kn = (const uint16_t *)c.Knew, a.Vn = (const uint16_t *)c.Vnew, a.Qo = (uint16_t *)c.Qout;
    a.Kc = (uint8_t *)c.Kc, a.Vc = (uint8_t *)c.Vc, a.kv_len = c.kv_len, a.inv_freq = c.inv_freq, a.wq = c.q_norm_w, a.wk = c.k_norm_w;
    a.ldq = c.ldq, a.ldk = c.ldk, a.ldv = c.ldv, a.ldqo = c.ldqo;
    a.tok_stride = c.tok_stride, a.head_stride = c.head_stride, a.seq_stride = c.seq_stride, a.T = c.B * c.N;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.n_head = (int)c.n_head, a.n_kv = (int)c.n_kv_head, a.n_rot = (int)c.n_rot;
    a.mscale = c.mscale, a.eps = c.eps;
    if (a.T == 0) return hipSuccess;
    a.rows4 = (((uintptr_t)c.Q | (uintptr_t)c.Knew | (uintptr_t)c.Vnew | (uintptr_t)c.Qout) & 3) == 0 &&
              ((c.ldq | c.ldk | c.ldv | c.ldqo) & 1) == 0;
    a.cache4 = (((uintptr_t)c.Kc | (uintptr_t)c.Vc | (uintptr_t)c.tok_stride | (uintptr_t)c.head_stride | (uintptr_t)c.seq_stride) & 3) == 0;
    // the shares of a token's head jobs: as many as fill the chip twice over, at most one pass each
    const int64_t J = c.n_head + 2 * c.n_kv_head, per_pass = c.D >= 128 ? 4 : 8, cus = num_cus();
    const int64_t ymax = (J + per_pass - 1) / per_pass, want = (2 * cus + a.T - 1) / a.T;
    const int64_t Y = want < 1 ? 1 : (want > ymax ? ymax : want);
    a.passes = (int)((ymax + Y - 1) / Y);
    const int64_t gy = (ymax + a.passes - 1) / a.passes, cap = 8 * cus;
    const dim3 grid((unsigned)(a.T < cap ? a.T : cap), (unsigned)gy), block(256);
    const bool norm = c.q_norm_w != nullptr;
#define GQ_ROPE(KV, D, MODE) \
    (norm ? rope_append_kernel<KV, D, MODE, true><<<grid, block, 0, s>>>(a) : rope_append_kernel<KV, D, MODE, false><<<grid, block, 0, s>>>(a))
#define GQ_ROPE256(KV, MODE) \
    (norm ? rope_append256_kernel<KV, MODE, true><<<grid, block, 0, s>>>(a) : rope_append256_kernel<KV, MODE, false><<<grid, block, 0, s>>>(a))
#define GQ_ROPE_D(KV, MODE) (c.D == 256 ? GQ_ROPE256(KV, MODE) : c.D == 128 ? GQ_ROPE(KV, 128, MODE) : GQ_ROPE(KV, 64, MODE))
    if (kv == 0) mode == 0 ? GQ_ROPE_D(0, 0) : GQ_ROPE_D(0, 1);
    else mode == 0 ? GQ_ROPE_D(1, 0) : GQ_ROPE_D(1, 1);
#undef GQ_ROPE_D
#undef GQ_ROPE256
#undef GQ_ROPE
    return hipGetLastError();
}

} // namespace gq

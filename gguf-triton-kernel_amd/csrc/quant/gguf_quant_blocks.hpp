// gguf_quant_blocks.hpp -- the GGUF block producers, one block at a time, for the host
// (gguf_quant.cpp, g++ -ffp-contract=off) and the device (quant_device.hip: one thread per
// block, the on-device requantization of SURVEY 8(f)2).  Every multiply/add is kept separately
// rounded in the reference's order (contraction off in both compilers), divisions and sqrt are
// IEEE (HIP's default correctly rounded fp32 divide/sqrt), so both give the reference's bytes;
// tests/golden/golden_quant.npz pins the host, tests/test_gpu_quant_device.py the device.
//
//   q4k_block  <- (GGML) quantize_row_q4_K_ref / make_qkx2_quants, q4_k_ref.c:188-368
//   q6k_block  <- (GGML) quantize_row_q6_K_ref / make_qx_quants, q6_k_ref.c:153-340
//   q5k_block  (no reference; host only) q4k_block's search with 31 levels, Q5_K packing
//   q3k_block  (no reference; host only) q6k_block's search over codes -4..3, Q3_K packing
//   q2k_block  (no reference; host only) q4k_block's scale / min fit per 16 elements over codes 0..3, Q2_K packing
//   q8_block   <- utils/quantize/q8_0.py:4-49 (Q8_0), utils/quantize/q8_1.py:18-70 (Q8_1)
//   q4_0_block (no reference; host and device) d = extreme / -8, codes by truncation of x/d + 8.5
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../gguf_half.hpp"

#ifdef __HIPCC__
#define GQ_QHD __host__ __device__
#else
#define GQ_QHD
#endif

#ifdef __clang__
#pragma clang fp contract(off)
#endif

namespace gq {
namespace qblk {

using gq::f2h;
using gq::h2f;

constexpr int QK = 256;
constexpr float kGroupMaxEps = 1e-15f;

// Round-to-nearest-even through the 1.5*2^23 magic constant; valid for |v| <= 2^22.
GQ_QHD inline int round_magic(float v)
{
    float t = v + 12582912.f;
    int32_t bits;
    __builtin_memcpy(&bits, &t, 4);
    return (bits & 0x007fffff) - 0x00400000;
}

GQ_QHD inline void put16(uint8_t *p, uint16_t v)
{
    p[0] = (uint8_t)(v & 0xff);
    p[1] = (uint8_t)(v >> 8);
}

GQ_QHD inline uint16_t get16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }

// ---------------- Q4_K ----------------
// Weighted fit of x ~ scale * L + min over L in [0, nmax] (GGML make_qkx2_quants with
// rmin=-1, rdelta=0.1, nstep=20, squared error).  Returns scale, writes -min to *neg_min.
// NMAX: the largest code (15: Q4_K, 31: Q5_K, 3: Q2_K).  N: elements per sub-block (Q2_K: 16).
template <int NMAX = 15, int N = 32>
GQ_QHD inline float fit_scale_min(const float *x, const float *w, uint8_t *L, uint8_t *Ltmp, float *neg_min)
{
    constexpr int n = N, nmax = NMAX, nstep = 20;
    constexpr float rmin = -1.f, rdelta = 0.1f;
    float lo = x[0], hi = x[0];
    float sw = w[0];
    float swx = sw * x[0];
    for (int i = 1; i < n; ++i) {
        lo = x[i] < lo ? x[i] : lo;
        hi = x[i] > hi ? x[i] : hi;
        float wi = w[i];
        sw += wi;
        swx += wi * x[i];
    }
    if (lo > 0) lo = 0;
    if (hi == lo) {
        __builtin_memset(L, 0, n);
        *neg_min = -lo;
        return 0.f;
    }
    float inv = nmax / (hi - lo);
    float scale = 1 / inv;
    float best = 0;
    for (int i = 0; i < n; ++i) {
        int l = round_magic(inv * (x[i] - lo));
        L[i] = (uint8_t)std::max(0, std::min(nmax, l));
        float e = scale * L[i] + lo - x[i];
        best += w[i] * (e * e);
    }
    for (int step = 0; step <= nstep; ++step) {
        float cand = (rmin + rdelta * step + nmax) / (hi - lo);
        float sl = 0, sl2 = 0, sxl = 0;
        for (int i = 0; i < n; ++i) {
            int l = round_magic(cand * (x[i] - lo));
            l = std::max(0, std::min(nmax, l));
            Ltmp[i] = (uint8_t)l;
            float wi = w[i];
            sl += wi * l;
            sl2 += wi * l * l;
            sxl += wi * l * x[i];
        }
        float det = sw * sl2 - sl * sl;
        if (det > 0) {
            float s = (sw * sxl - swx * sl) / det;
            float m = (sl2 * swx - sl * sxl) / det;
            if (m > 0) {
                m = 0;
                s = sxl / sl2;
            }
            float err = 0;
            for (int i = 0; i < n; ++i) {
                float e = s * Ltmp[i] + m - x[i];
                err += w[i] * (e * e);
            }
            if (err < best) {
                __builtin_memcpy(L, Ltmp, n);
                best = err;
                scale = s;
                lo = m;
            }
        }
    }
    *neg_min = -lo;
    return scale;
}

GQ_QHD inline void q4k_block(const float *x, uint8_t *blk)
{
    uint8_t L[QK], Ltmp[32];
    float w[32], sub_scale[8], sub_min[8];
    float max_scale = 0, max_min = 0;
    for (int j = 0; j < 8; ++j) {
        const float *xs = x + 32 * j;
        float ss = 0;
        for (int l = 0; l < 32; ++l) ss += xs[l] * xs[l];
        float rms = std::sqrt(ss / 32);
        for (int l = 0; l < 32; ++l) w[l] = rms + std::fabs(xs[l]);
        sub_scale[j] = fit_scale_min(xs, w, L + 32 * j, Ltmp, &sub_min[j]);
        if (sub_scale[j] > max_scale) max_scale = sub_scale[j];
        if (sub_min[j] > max_min) max_min = sub_min[j];
    }
    float inv_s = max_scale > 0 ? 63.f / max_scale : 0.f;
    float inv_m = max_min > 0 ? 63.f / max_min : 0.f;
    uint8_t *sc = blk + 4;
    __builtin_memset(sc, 0, 12);
    for (int j = 0; j < 8; ++j) {
        uint8_t ls = (uint8_t)round_magic(inv_s * sub_scale[j]);
        uint8_t lm = (uint8_t)round_magic(inv_m * sub_min[j]);
        ls = std::min<uint8_t>(63, ls);
        lm = std::min<uint8_t>(63, lm);
        if (j < 4) {
            sc[j] = ls;
            sc[j + 4] = lm;
        } else {
            sc[j + 4] = (uint8_t)((ls & 0x0f) | ((lm & 0x0f) << 4));
            sc[j - 4] |= (uint8_t)((ls >> 4) << 6);
            sc[j] |= (uint8_t)((lm >> 4) << 6);
        }
    }
    uint16_t dh = f2h(max_scale / 63.f), mh = f2h(max_min / 63.f);
    put16(blk, dh);
    put16(blk + 2, mh);
    for (int j = 0; j < 8; ++j) {
        int s6, m6;
        if (j < 4) {
            s6 = sc[j] & 63;
            m6 = sc[j + 4] & 63;
        } else {
            s6 = (sc[j + 4] & 0x0f) | ((sc[j - 4] >> 6) << 4);
            m6 = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4);
        }
        float d = h2f(dh) * s6;
        if (!d) continue;
        float dm = h2f(mh) * m6;
        for (int i = 0; i < 32; ++i) {
            int l = round_magic((x[32 * j + i] + dm) / d);
            L[32 * j + i] = (uint8_t)std::max(0, std::min(15, l));
        }
    }
    uint8_t *qs = blk + 16;
    for (int c = 0; c < 4; ++c)
        for (int l = 0; l < 32; ++l) qs[32 * c + l] = (uint8_t)(L[64 * c + l] | (L[64 * c + 32 + l] << 4));
}

// ---------------- Q5_K ----------------
// Q4_K's producer with codes 0..31: the same per-sub-block scale / min search (fit_scale_min<31>),
// the same 6-bit scale / min packing and header; the codes' low nibbles in qs [48:176] as Q4_K's,
// bit 4 of sub-block j's element l in bit j of qh[l] [16:48].
GQ_QHD inline void q5k_block(const float *x, uint8_t *blk)
{
    uint8_t L[QK], Ltmp[32];
    float w[32], sub_scale[8], sub_min[8];
    float max_scale = 0, max_min = 0;
    for (int j = 0; j < 8; ++j) {
        const float *xs = x + 32 * j;
        float ss = 0;
        for (int l = 0; l < 32; ++l) ss += xs[l] * xs[l];
        float rms = std::sqrt(ss / 32);
        for (int l = 0; l < 32; ++l) w[l] = rms + std::fabs(xs[l]);
        sub_scale[j] = fit_scale_min<31>(xs, w, L + 32 * j, Ltmp, &sub_min[j]);
        if (sub_scale[j] > max_scale) max_scale = sub_scale[j];
        if (sub_min[j] > max_min) max_min = sub_min[j];
    }
    float inv_s = max_scale > 0 ? 63.f / max_scale : 0.f;
    float inv_m = max_min > 0 ? 63.f / max_min : 0.f;
    uint8_t *sc = blk + 4;
    __builtin_memset(sc, 0, 12);
    for (int j = 0; j < 8; ++j) {
        uint8_t ls = (uint8_t)round_magic(inv_s * sub_scale[j]);
        uint8_t lm = (uint8_t)round_magic(inv_m * sub_min[j]);
        ls = std::min<uint8_t>(63, ls);
        lm = std::min<uint8_t>(63, lm);
        if (j < 4) {
            sc[j] = ls;
            sc[j + 4] = lm;
        } else {
            sc[j + 4] = (uint8_t)((ls & 0x0f) | ((lm & 0x0f) << 4));
            sc[j - 4] |= (uint8_t)((ls >> 4) << 6);
            sc[j] |= (uint8_t)((lm >> 4) << 6);
        }
    }
    uint16_t dh = f2h(max_scale / 63.f), mh = f2h(max_min / 63.f);
    put16(blk, dh);
    put16(blk + 2, mh);
    for (int j = 0; j < 8; ++j) {
        int s6, m6;
        if (j < 4) {
            s6 = sc[j] & 63;
            m6 = sc[j + 4] & 63;
        } else {
            s6 = (sc[j + 4] & 0x0f) | ((sc[j - 4] >> 6) << 4);
            m6 = (sc[j + 4] >> 4) | ((sc[j] >> 6) << 4);
        }
        float d = h2f(dh) * s6;
        if (!d) continue;
        float dm = h2f(mh) * m6;
        for (int i = 0; i < 32; ++i) {
            int l = round_magic((x[32 * j + i] + dm) / d);
            L[32 * j + i] = (uint8_t)std::max(0, std::min(31, l));
        }
    }
    uint8_t *qh = blk + 16, *qs = blk + 48;
    __builtin_memset(qh, 0, 32);
    for (int c = 0; c < 4; ++c)
        for (int l = 0; l < 32; ++l) {
            const uint8_t a = L[64 * c + l], b = L[64 * c + 32 + l];
            qs[32 * c + l] = (uint8_t)((a & 0x0f) | ((b & 0x0f) << 4));
            qh[l] |= (uint8_t)(((a >> 4) << (2 * c)) | ((b >> 4) << (2 * c + 1)));
        }
}

// ---------------- Q6_K ----------------
// Symmetric fit x ~ scale * l, l in [-32, 31], squared-x weights
// (GGML make_qx_quants with nmax=32, rmse_type=1).  L receives l + 32.
// NMAX: codes in [-NMAX, NMAX - 1], L receives l + NMAX (32: Q6_K, 4: Q3_K).  W2 = false: plain
// squared error (Q3_K: no squared-x weights).
template <int NMAX = 32, bool W2 = true>
GQ_QHD inline float fit_scale_sym(const float *x, int8_t *L)
{
    constexpr int n = 16, nmax = NMAX;
    float peak = 0, amax = 0;
    for (int i = 0; i < n; ++i) {
        float a = std::fabs(x[i]);
        if (a > amax) {
            amax = a;
            peak = x[i];
        }
    }
    if (amax < kGroupMaxEps) {
        __builtin_memset(L, 0, n);
        return 0.f;
    }
    float inv = -nmax / peak;
    float sxl = 0, sl2 = 0;
    for (int i = 0; i < n; ++i) {
        int l = round_magic(inv * x[i]);
        l = std::max(-nmax, std::min(nmax - 1, l));
        L[i] = (int8_t)(l + nmax);
        float w = W2 ? x[i] * x[i] : 1.f;
        sxl += w * x[i] * l;
        sl2 += w * l * l;
    }
    float scale = sl2 ? sxl / sl2 : 0.0f;
    float best = scale * sxl;
    for (int step = -9; step <= 9; ++step) {
        if (step == 0) continue;
        float cand = -(nmax + 0.1f * step) / peak;
        float a = 0, b = 0;
        for (int i = 0; i < n; ++i) {
            int l = round_magic(cand * x[i]);
            l = std::max(-nmax, std::min(nmax - 1, l));
            float w = W2 ? x[i] * x[i] : 1.f;
            a += w * x[i] * l;
            b += w * l * l;
        }
        if (b > 0 && a * a > best * b) {
            for (int i = 0; i < n; ++i) {
                int l = round_magic(cand * x[i]);
                L[i] = (int8_t)(nmax + std::max(-nmax, std::min(nmax - 1, l)));
            }
            scale = a / b;
            best = scale * a;
        }
    }
    return scale;
}

GQ_QHD inline void q6k_block(const float *x, uint8_t *blk)
{
    int8_t L[QK];
    float sub[16];
    float max_scale = 0, max_abs = 0;
    for (int ib = 0; ib < 16; ++ib) {
        sub[ib] = fit_scale_sym(x + 16 * ib, L + 16 * ib);
        float a = std::fabs(sub[ib]);
        if (a > max_abs) {
            max_abs = a;
            max_scale = sub[ib];
        }
    }
    __builtin_memset(blk, 0, 210);
    if (max_abs < kGroupMaxEps) {
        put16(blk + 208, f2h(0.f));
        return;
    }
    float inv = -128.f / max_scale;
    uint16_t dh = f2h(1 / inv);
    put16(blk + 208, dh);
    int8_t *scales = (int8_t *)(blk + 192);
    for (int ib = 0; ib < 16; ++ib) scales[ib] = (int8_t)std::min(127, round_magic(inv * sub[ib]));
    for (int j = 0; j < 16; ++j) {
        float d = h2f(dh) * scales[j];
        if (!d) continue;
        for (int i = 0; i < 16; ++i) {
            int l = round_magic(x[16 * j + i] / d);
            L[16 * j + i] = (int8_t)(std::max(-32, std::min(31, l)) + 32);
        }
    }
    uint8_t *ql = blk, *qh = blk + 128;
    for (int half = 0; half < 2; ++half) {
        const int8_t *Lh = L + 128 * half;
        for (int l = 0; l < 32; ++l) {
            uint8_t a = (uint8_t)Lh[l], b = (uint8_t)Lh[l + 32], c = (uint8_t)Lh[l + 64], d = (uint8_t)Lh[l + 96];
            ql[64 * half + l] = (uint8_t)((a & 0x0f) | ((c & 0x0f) << 4));
            ql[64 * half + l + 32] = (uint8_t)((b & 0x0f) | ((d & 0x0f) << 4));
            qh[32 * half + l] = (uint8_t)((a >> 4) | ((b >> 4) << 2) | ((c >> 4) << 4) | ((d >> 4) << 6));
        }
    }
}

// ---------------- Q3_K ----------------
// Q6_K's producer with codes -4..3: per 16 elements the symmetric scale search (fit_scale_sym<4, false>: plain squared error),
// the sixteen scales quantized to 6 bits (-32..31) against the one of largest magnitude, which
// takes -32; then the codes re-fitted to the quantized scales.  Packing: include/gguf_mmq.h.
GQ_QHD inline void q3k_block(const float *x, uint8_t *blk)
{
    int8_t L[QK];
    float sub[16];
    float max_scale = 0, max_abs = 0;
    for (int ib = 0; ib < 16; ++ib) {
        sub[ib] = fit_scale_sym<4, false>(x + 16 * ib, L + 16 * ib);
        float a = std::fabs(sub[ib]);
        if (a > max_abs) {
            max_abs = a;
            max_scale = sub[ib];
        }
    }
    __builtin_memset(blk, 0, 110);
    int sc[16];
    if (max_abs < kGroupMaxEps) { // all codes -4 + 4 = hmask set, scales 0 (stored 32), d = 0: zeros
        for (int ib = 0; ib < 16; ++ib) sc[ib] = 0;
        for (int i = 0; i < QK; ++i) L[i] = 4;
        put16(blk + 108, f2h(0.f));
    } else {
        float inv = -32.f / max_scale;
        uint16_t dh = f2h(1 / inv);
        put16(blk + 108, dh);
        for (int ib = 0; ib < 16; ++ib) sc[ib] = std::max(-32, std::min(31, round_magic(inv * sub[ib])));
        for (int j = 0; j < 16; ++j) {
            float d = h2f(dh) * sc[j];
            if (!d) continue;
            for (int i = 0; i < 16; ++i) {
                int l = round_magic(x[16 * j + i] / d);
                L[16 * j + i] = (int8_t)(std::max(-4, std::min(3, l)) + 4);
            }
        }
    }
    uint8_t *hm = blk, *qs = blk + 32, *scales = blk + 96;
    for (int s = 0; s < 16; ++s) {
        const int v = sc[s] + 32; // 0..63
        if (s < 8) scales[s] |= (uint8_t)(v & 15);
        else scales[s - 8] |= (uint8_t)((v & 15) << 4);
        scales[8 + s % 4] |= (uint8_t)((v >> 4) << (2 * (s / 4)));
    }
    for (int e = 0; e < QK; ++e) {
        const int h = e / 128, j = (e % 128) / 32, l = e % 32, c = L[e];
        qs[32 * h + l] |= (uint8_t)((c & 3) << (2 * j));
        hm[l] |= (uint8_t)((c >> 2) << (4 * h + j));
    }
}

// ---------------- Q2_K ----------------
// Per 16 elements a scale and a non-negative min over codes 0..3 (fit_scale_min<3, 16>, plain
// squared error: all weights 1); the sixteen scales and the sixteen mins quantized to 4 bits against
// the largest of each (d = max scale / 15, dmin = max min / 15); then the codes re-fitted to the
// quantized scales and mins.  Packing: include/gguf_mmq.h.
GQ_QHD inline void q2k_block(const float *x, uint8_t *blk)
{
    uint8_t L[QK], Ltmp[16];
    float w[16], sub_scale[16], sub_min[16];
    float max_scale = 0, max_min = 0;
    for (int l = 0; l < 16; ++l) w[l] = 1.f;
    for (int j = 0; j < 16; ++j) {
        sub_scale[j] = fit_scale_min<3, 16>(x + 16 * j, w, L + 16 * j, Ltmp, &sub_min[j]);
        if (sub_scale[j] > max_scale) max_scale = sub_scale[j];
        if (sub_min[j] > max_min) max_min = sub_min[j];
    }
    const float inv_s = max_scale > 0 ? 15.f / max_scale : 0.f;
    const float inv_m = max_min > 0 ? 15.f / max_min : 0.f;
    const uint16_t dh = f2h(max_scale / 15.f), mh = f2h(max_min / 15.f);
    __builtin_memset(blk, 0, 84);
    put16(blk + 80, dh);
    put16(blk + 82, mh);
    uint8_t *scales = blk, *qs = blk + 16;
    for (int j = 0; j < 16; ++j) {
        const int ls = std::max(0, std::min(15, round_magic(inv_s * sub_scale[j])));
        const int lm = std::max(0, std::min(15, round_magic(inv_m * sub_min[j])));
        scales[j] = (uint8_t)(ls | (lm << 4));
        const float d = h2f(dh) * ls;
        if (!d) { // (a zero scale: the codes carry nothing, the min alone stands for the sub-block)
            for (int i = 0; i < 16; ++i) L[16 * j + i] = 0;
            continue;
        }
        const float dm = h2f(mh) * lm;
        for (int i = 0; i < 16; ++i) {
            int l = round_magic((x[16 * j + i] + dm) / d);
            L[16 * j + i] = (uint8_t)std::max(0, std::min(3, l));
        }
    }
    for (int e = 0; e < QK; ++e) {
        const int h = e / 128, j = (e % 128) / 32, l = e % 32;
        qs[32 * h + l] |= (uint8_t)(L[e] << (2 * j));
    }
}

// ---------------- Q8_0 / Q8_1 (the reference's torch producers, fp16 arithmetic) ----------------
// d = fp16(amax / 127); q = clamp(rne(fp16(x / d)), +-127).  Q8_0 stores d = 1 for an all-zero
// block; Q8_1 stores d = 0 there (dividing by 1) and s = fp16(d * fp16(sum q)).
template <bool WITH_SUM>
GQ_QHD inline void q8_block(const uint16_t *x, uint8_t *blk)
{
    float amax = 0.f;
    for (int i = 0; i < 32; ++i) amax = std::max(amax, std::fabs(h2f(x[i])));
    uint16_t d = WITH_SUM ? (uint16_t)0 : (uint16_t)0x3c00;
    if (amax != 0.f) d = f2h(amax / 127.0f);
    float div = h2f(d);
    if (WITH_SUM && div == 0.f) div = 1.f;
    uint8_t *qs = blk + (WITH_SUM ? 4 : 2);
    int32_t sum = 0;
    for (int i = 0; i < 32; ++i) {
        float q = std::nearbyint(h2f(f2h(h2f(x[i]) / div)));
        if (q != q) q = 0.f; // 0/0 when d underflowed to 0 (tiny Q8_0 block): torch's int8 cast gives 0
        q = std::min(127.f, std::max(-127.f, q));
        int8_t qi = (int8_t)q;
        qs[i] = (uint8_t)qi;
        sum += qi;
    }
    put16(blk, d);
    if (WITH_SUM) put16(blk + 2, f2h(h2f(d) * h2f(f2h((float)sum))));
}

// ---------------- Q4_0 ----------------
// 32 weights in 18 bytes: fp16 d, then qs[16] (element j in the low nibble of qs[j], element 16 + j
// in the high one); w = d*(q - 8).  The rule: m = the element of largest magnitude, sign kept;
// d = m / -8, id = d ? 1/d : 0; q = min(15, (int)(x*id + 8.5f)) (x*id >= -8 up to a rounding, so the
// truncation is a rounding to nearest and m itself gets code 0); d stored as fp16.
GQ_QHD inline void q4_0_block(const float *x, uint8_t *blk)
{
    float amax = 0.f, mx = 0.f;
    for (int i = 0; i < 32; ++i) {
        const float v = x[i];
        if (amax < std::fabs(v)) {
            amax = std::fabs(v);
            mx = v;
        }
    }
    const float d = mx / -8.f;
    const float id = d != 0.f ? 1.f / d : 0.f;
    put16(blk, f2h(d));
    for (int j = 0; j < 16; ++j) {
        const float x0 = x[j] * id, x1 = x[16 + j] * id;
        const int q0 = std::min(15, (int)(int8_t)(x0 + 8.5f)), q1 = std::min(15, (int)(int8_t)(x1 + 8.5f));
        blk[2 + j] = (uint8_t)(q0 | (q1 << 4));
    }
}

} // namespace qblk
} // namespace gq

// attn_mla_proj.hip -- the two per-head latent projections around DeepSeek's absorbed attention
// (gq_mla_proj): dir 0 absorbs W_UK into q_nope (Y = the first 512 of every 576-wide head of gq_mla_decode's
// Q), dir 1 expands the attention output by W_UV (Y = attn_output's input).  Both are Y_h = X_h W_h^T with
// W_h a row-major Mo x Kc fp16 matrix, contraction index contiguous:
//
//   dir 0  absorb  W_UK (n_head, 512, 128)  Mo = 512  Kc = 128
//   dir 1  expand  W_UV (n_head, 128, 512)  Mo = 128  Kc = 512
//
//   Y[t*ldy + h*y_head_stride + m] = fp16( sum_k X[t*ldx + h*x_head_stride + k] * W[(h*Mo + m)*Kc + k] )
//
// fp16 products (exact in fp32), fp32 accumulation on v_mfma_f32_16x16x32_f16, one rounding.  Nothing but
// the Mo values of every (t, h) is written: the rotated q_pe gq_mla_append left in columns 512..575 of
// every head of the same buffer survives an absorb.  No reference counterpart.
//
// Operands.  D^T = W X^T: the A operand is a 16-row tile of W (lane (g, c) = lane >> 4, lane & 15 holds
// W[m0 + c][k0 + 8 g .. + 7], one 16-byte piece), the B operand 16 tokens of X (lane (g, c): token c, the
// same 8 k), so acc element i of lane (g, c) is Y[token c][m0 + 4 g + i]: four consecutive outputs, one
// 8-byte store.  A token's column of the MFMA depends on no other token; rows beyond T are zero fragments
// and are not stored.
//
// Two forms; the host picks one from T and n_head alone (plan_mla_proj), never from device data.
//
// Few-row form (T <= 16: decode).  The work is streaming W once.  Every wave covers a 128-wide range of k
// -- all of absorb's Kc, a quarter of expand's -- so its X fragments are four registers-of-8 (16 VGPRs) for
// the whole kernel, and per 16-row tile of W it issues four 16-byte loads per lane straight into the A
// operand (a row's four lanes g read 64 contiguous bytes, two k-steps complete a 128-byte line) and four
// MFMAs.  Absorb: a workgroup is ONE wave with TPW tiles (grid n_head * 32 / TPW).  Expand: a workgroup is
// FOUR waves that split Kc over the same TPW tiles, write their fp32 partials to LDS (4 KiB per tile) and
// waves 0 .. TPW - 1 sum them in a fixed order and store (grid n_head * 8 / TPW).  TPW is 2 from 64 heads
// (128 heads: 2048 / 512 workgroups) and 1 below (16 heads: 512 / 128 workgroups, every 16-row tile its
// own).  No atomics, no workspace.  All of a wave's W loads are issued before the first MFMA.
//
// Tiled form (T > 16: prefill).  One workgroup of four waves per (head, 64 tokens), wave v the 16-token
// tile 16 v .. 16 v + 15 as in mla_prefill_kernel; the X fragments of the wave's 16 tokens stay in
// registers (absorb 4, expand 16 registers-of-8).  The head's 128 KiB of W is walked in eight 16 KiB
// stages of contiguous memory -- 64 rows of absorb's 256-byte rows (four 16-row tiles), 16 rows of
// expand's 1024-byte rows (one tile) -- that the four waves share through an LDS ring of three slots
// (48 KiB) filled by LDS-DMA: per stage s_waitcnt vmcnt(4) (this wave's four pieces of stage s; those of
// stage s + 1 may still fly), ONE barrier, issue stage s + 2 into stage s - 1's slot, 16 MFMAs, store.
// Y's stores count in vmcnt too: that only makes the wait stricter (loads return in order among
// themselves, so four outstanding operations can never include a piece of stage s).  Issues past the last
// stage go outside the buffer resource: zeros, no access, the same count at the tail.  Piece p of row r
// lands at LDS piece p ^ (r & 15) of its row, so the 16 rows c of a fragment read (same g) fall on 16
// distinct 16-byte bank groups.  Workgroups of one head are neighbours (id = head * tiles + tile): W_h
// is fetched from HBM once and re-read from L2.  Per stage a wave reads 16 KiB from LDS for 16 MFMAs: four
// waves, 64 KiB at 128 B/clk = 512 clocks against 16 x 16 = 256 of MFMA per SIMD, so the form is
// LDS-bound by about 2x (reasoned from public peak figures); two token tiles per wave would balance it.
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"

namespace gq {
namespace {

struct MlaProjArgs {
    const uint16_t *W, *X;
    uint16_t *Y;
    int64_t ldx, xhs, ldy, yhs;
    int T, ntile; // ntile: 64-token tiles (tiled form)
};

template <int DIR> struct Proj {
    static constexpr int MO = DIR ? kMlaProjDim : kMlaRank, KC = DIR ? kMlaRank : kMlaProjDim;
    static constexpr int KW = KC / 128;            // few-row: waves of a workgroup, each 128 k
    static constexpr int KS = KC / 32;             // tiled: k-steps
    static constexpr int PPR = KC / 8;             // 16-byte pieces per row of W
    static constexpr int MT = kMlaProjStageB / (16 * 2 * KC); // tiled: 16-row tiles per stage
    static constexpr int NST = MO / (16 * MT);     // stages per head
    static_assert(NST * kMlaProjStageB == 2 * MO * KC && MT * KS == 16, "a stage is 16 KiB: 16 MFMAs");
};

__device__ __forceinline__ void store4(uint16_t *dst, const f32x4 v)
{
    *(u32x2 *)dst = (u32x2){(uint32_t)f2h_bits(v[0]) | ((uint32_t)f2h_bits(v[1]) << 16),
                            (uint32_t)f2h_bits(v[2]) | ((uint32_t)f2h_bits(v[3]) << 16)};
}

template <int DIR, int TPW>
__global__ __launch_bounds__(64 * Proj<DIR>::KW) void mla_proj_few_kernel(const MlaProjArgs a)
{
    using P = Proj<DIR>;
    constexpr int UPH = P::MO / (16 * TPW); // workgroups per head
    const int lane = threadIdx.x & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = blockIdx.x / UPH, m0 = (blockIdx.x % UPH) * (16 * TPW), k0 = 128 * wave + 8 * g;
    const bool live = c < a.T;

    u32x4 wf[TPW][4], xv[4];
    const uint16_t *w = a.W + ((int64_t)h * P::MO + m0 + c) * P::KC + k0;
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) wf[j][s] = ld16(w + 16 * j * P::KC + 32 * s);
    const uint16_t *x = a.X + (live ? c : 0) * a.ldx + h * a.xhs + k0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        xv[s] = (u32x4){0, 0, 0, 0};
        if (live) xv[s] = ld16(x + 32 * s);
    }

    f32x4 acc[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j) {
        acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[j][s]), __builtin_bit_cast(f16x8, xv[s]),
                                                            acc[j], 0, 0, 0);
    }

    uint16_t *y = a.Y + (live ? c : 0) * a.ldy + h * a.yhs + m0 + 4 * g;
    if constexpr (P::KW == 1) {
        if (live) {
#pragma unroll
            for (int j = 0; j < TPW; ++j) store4(y + 16 * j, acc[j]);
        }
    } else {
        __shared__ f32x4 part[P::KW][TPW][64];
#pragma unroll
        for (int j = 0; j < TPW; ++j) part[wave][j][lane] = acc[j];
        __syncthreads();
        if (wave < TPW && live) { // (wave-uniform, then the live tokens) the k quarters in their order
            f32x4 v = part[0][wave][lane];
#pragma unroll
            for (int q = 1; q < P::KW; ++q) v += part[q][wave][lane];
            store4(y + 16 * wave, v);
        }
    }
}

template <int DIR>
__global__ __launch_bounds__(256) void mla_proj_tiled_kernel(const MlaProjArgs a)
{
    using P = Proj<DIR>;
    constexpr int NI = kMlaProjStageB / (16 * 256); // 4 DMAs per lane and stage
    __shared__ __attribute__((aligned(256))) uint8_t smem[kMlaProjSlots * kMlaProjStageB];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x / (unsigned)a.ntile, tile = blockIdx.x % (unsigned)a.ntile;
    const int t = 64 * tile + 16 * wave + c;
    const bool live = t < a.T;

    // ---- X fragments of the wave's 16 tokens ----
    f16x8 xf[P::KS];
    {
        const uint16_t *x = a.X + (int64_t)(live ? t : 0) * a.ldx + h * a.xhs + 8 * g;
#pragma unroll
        for (int s = 0; s < P::KS; ++s) {
            u32x4 v = {0, 0, 0, 0};
            if (live) v = ld16(x + 32 * s);
            xf[s] = __builtin_bit_cast(f16x8, v);
        }
    }

    // ---- the lane's NI pieces of a stage's DMA: LDS piece 256 k + tid <- piece pos ^ (row & 15) of its row ----
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(a.W + (int64_t)h * P::MO * P::KC), 0, 2 * P::MO * P::KC, 0x00020000);
    uint32_t doff[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int q = 256 * k + tid, r = q / P::PPR, pos = q % P::PPR;
        doff[k] = 16u * (uint32_t)(r * P::PPR + (pos ^ (r & 15)));
    }
    auto issue = [&](int st) { // stage st into slot st % kMlaProjSlots; st >= NST: zeros, the same count
        uint8_t *dst = smem + (st % kMlaProjSlots) * kMlaProjStageB + 1024 * wave;
#pragma unroll
        for (int k = 0; k < NI; ++k)
            dma16(rs, dst + 4096 * k, st < P::NST ? (uint32_t)st * kMlaProjStageB + doff[k] : 0x80000000u, 0);
    };
    // fragment (mt, s) of a stage: row 16 mt + c, piece 4 s + g
    const uint32_t fbase = (uint32_t)(c * 2 * P::KC);
    uint16_t *y = a.Y + (int64_t)(live ? t : 0) * a.ldy + h * a.yhs + 4 * g;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // X has arrived: from here vmcnt counts DMAs (and Y's stores)
#pragma unroll
    for (int s = 0; s < P::KS; ++s) asm volatile("" : "+v"(xf[s]));
#pragma unroll
    for (int s = 0; s < kMlaProjSlots - 1; ++s) issue(s);
#pragma unroll
    for (int st = 0; st < P::NST; ++st) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI * (kMlaProjSlots - 2)) : "memory"); // this wave's pieces of stage st
        // stage st has landed; st - 1's slot is drained (its fragments were consumed by MFMAs).  The bare
        // barrier, not __syncthreads(): that one's release fence makes the compiler wait for vmcnt(0) --
        // the pieces of stage st + 1 and Y's stores -- before every barrier, and the ring would hold one
        // stage in flight, not two.  The wait above is what orders the DMA; the clobbers keep the compiler's
        // LDS reads below it.
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue(st + kMlaProjSlots - 1);
        const uint32_t S = (st % kMlaProjSlots) * kMlaProjStageB;
        f32x4 acc[P::MT];
#pragma unroll
        for (int mt = 0; mt < P::MT; ++mt) {
            acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < P::KS; ++s) {
                const f16x8 wf = __builtin_bit_cast(f16x8, *(const u32x4 *)(smem + S + fbase + 16 * mt * 2 * P::KC + 16 * ((4 * s + g) ^ c)));
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[s], acc[mt], 0, 0, 0);
            }
        }
        if (live) {
#pragma unroll
            for (int mt = 0; mt < P::MT; ++mt) store4(y + 16 * (P::MT * st + mt), acc[mt]);
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the trailing (empty) stages have landed
}

} // namespace

MlaProjPlan plan_mla_proj(int dir, int64_t T, int64_t n_head)
{
    MlaProjPlan p;
    if ((dir != 0 && dir != 1) || T <= 0 || n_head <= 0 || n_head > kMlaMaxHeads || T > INT32_MAX / n_head) return p;
    const int mo = dir ? kMlaProjDim : kMlaRank;
    if (T <= kMlaProjFewRows) {
        p.form = 0, p.rows = kMlaProjFewRows, p.tpw = n_head >= 64 ? 2 : 1;
        p.grid = n_head * (mo / (16 * p.tpw));
    } else {
        p.form = 1, p.rows = kMlaProjTileRows;
        p.grid = n_head * ((T + kMlaProjTileRows - 1) / kMlaProjTileRows);
    }
    p.ok = true;
    return p;
}

hipError_t launch_mla_proj(int dir, const MlaProjCall &c, const MlaProjPlan &p, hipStream_t s)
{
    MlaProjArgs a{};
    a.W = (const uint16_t *)c.W, a.X = (const uint16_t *)c.X, a.Y = (uint16_t *)c.Y;
    a.ldx = c.ldx, a.xhs = c.x_head_stride, a.ldy = c.ldy, a.yhs = c.y_head_stride;
    a.T = (int)c.T, a.ntile = (int)(p.grid / c.n_head);
    const dim3 grid((unsigned)p.grid);
    if (p.form == 1) {
        if (dir) mla_proj_tiled_kernel<1><<<grid, dim3(256), 0, s>>>(a);
        else mla_proj_tiled_kernel<0><<<grid, dim3(256), 0, s>>>(a);
    } else if (dir) {
        if (p.tpw == 2) mla_proj_few_kernel<1, 2><<<grid, dim3(256), 0, s>>>(a);
        else mla_proj_few_kernel<1, 1><<<grid, dim3(256), 0, s>>>(a);
    } else {
        if (p.tpw == 2) mla_proj_few_kernel<0, 2><<<grid, dim3(64), 0, s>>>(a);
        else mla_proj_few_kernel<0, 1><<<grid, dim3(64), 0, s>>>(a);
    }
    return hipGetLastError();
}

} // namespace gq

// attn_mla_prefill.hip -- DeepSeek's absorbed multi-head latent attention of the N tokens last appended
// to each sequence over that sequence's fp16 latent cache, for any N (gq_mla_prefill): a prompt, a chunk
// of one after a prefix, a speculative verification.  The cache row [c_kv (512) | k_pe (64)], the row
// order (row r = token r / n_head, head r % n_head), the kv_len semantics, the buffer-resource bounds
// and the arithmetic are attn_mla.hip's (gq_mla_decode); the work split is attn_prefill.hip's, whose
// header has the arguments.  The tile geometry, the swizzle and the DMA addressing are gguf_mla.hpp's.
// No reference counterpart.
//
// Work split.  One launch, no workspace, no combine, nothing split along the keys.  A workgroup of 4
// waves owns kMlaPrefillRows = 64 consecutive rows of one sequence; wave v owns the 16-row MFMA tile
// 16 v .. 16 v + 15 of the block -- its Q fragments (18 k-steps x 4 registers), its O^T accumulators (32
// column groups x 4 fp32) and its online softmax never leave its registers -- and finishes their softmax
// alone; O is rounded to fp16 once and stored.  The grid, B * ceil(R / 64), depends on no length;
// workgroup ids count the row blocks from the last one down (all sequences of the last block first), so
// the blocks with the most keys start first and the short ones fill the tail.  attn_mla.hip's die-aware
// id order is dropped: it served several row groups streaming one share of a long cache at the same
// time, and here a sequence's blocks walk different key ranges at different times.  Unmeasured either way.
//
// Why 16 rows per wave and not 32.  With 16 rows a wave reads, per 32-key tile, 36 KiB of K fragments
// and 32 KiB of V^T fragments from LDS for 68 MFMAs: four waves, 272 KiB at 128 B/clk, about 2200 clocks
// against 68 x 16 = 1100 of MFMA per SIMD -- LDS-bound by about 2x once the products are the cost (at
// decode the cache stream is).  Two 16-row tiles per wave sharing every fragment (attn_prefill.hip's RT =
// 2) would balance the two pipes, and that form was written first: this kernel with every per-row
// quantity doubled, all of Q in registers.  O^T is then 256 registers and Q 144 of the 512, and the
// compiler could not hold it: 256 VGPRs + 256 AGPRs and 988 bytes of scratch per lane (255 spilled
// registers), 524 bytes with the rescale unconditional, no causal skip and no scheduling directives --
// Q itself goes to scratch, and scratch accesses would also break the vmcnt count the ring relies on.
// Re-reading Q's k_pe part from LDS buys 16 registers of the ~140 missing.  So the 16-row form ships
// (256 VGPRs + 138 AGPRs, no scratch); a 32-row form needs Q out of the registers (a 64-row workgroup
// whose waves split O's columns and exchange P through LDS) and is the next step.  DESIGN.md has the
// reports.  (The clock figures are reasoned from public peak figures, not measured.)
//
// Ring.  attn_mla.hip's: kMlaSlots = 3 slots of one 36 KiB tile, 108 KiB of the 160.  Per tile i:
// s_waitcnt vmcnt(9) (the wave's pieces of tile i; those of tile i + 1 may still fly), ONE workgroup
// barrier, issue tile i + 2 into tile i - 1's slot, compute tile i.  Issues past the last tile go
// outside the buffer resource (zeros, no access), so the count the wait relies on is the same at the tail.
//
// Causality is skipped, not only masked.  A workgroup walks the tiles up to its last row's limit and
// fetches no key beyond it; a wave skips the MFMAs of a tile wholly beyond its own last row's limit
// (wave-uniform; it still issues its DMA share and meets the barrier), and the per-element compare
// runs only in tiles that reach beyond the wave's FIRST row's limit.  With 64 or 128 heads a wave's 16 rows are
// one token's and its limit is uniform; with 16 or 20 heads a block spans several tokens.
//
// Rows at or beyond a block's key count and the issues past its tiles get a DMA offset outside the
// buffer resource: zeros, no access, so a dead row's bytes (NaN included) never reach an MFMA.  A live
// key beyond a row's own limit is masked to p = exactly 0.
#include "gguf_attn.hpp"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"
#include "gguf_mla.hpp"

namespace gq {
namespace {

constexpr float kNegInf = -__builtin_huge_valf();
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct MlaPrefillArgs {
    const uint16_t *Q;
    const uint8_t *C;
    const int32_t *kv_len;
    uint16_t *O;
    int64_t ldq, ldo, tok_stride, seq_stride;
    int capacity, N, n_head, nblk, B, o8;
    float c; // scale * log2(e): scores are kept in the exp2 domain
};

__global__ __launch_bounds__(256) void mla_prefill_kernel(const MlaPrefillArgs a)
{
    constexpr int WR = 16, ROWS = kMlaPrefillRows, KS = kMlaKS, NG = kMlaNG, NI = kMlaNI;
    static_assert(ROWS == kMlaWaves * WR, "one 16-row MFMA tile per wave");
    __shared__ __attribute__((aligned(256))) uint8_t smem[kMlaSlots * kMlaTileB];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the last row block (the most keys) first
    const int rb = a.nblk - 1 - (int)(blockIdx.x / (unsigned)a.B), b = (int)(blockIdx.x % (unsigned)a.B);
    const int R = a.N * a.n_head;
    int len = a.kv_len[b];
    len = len < 0 ? 0 : (len > a.capacity ? a.capacity : len); // never outside the cache
    // keys the block's last row attends (0: none of its rows attends anything), and the wave's own limits
    const int r0 = rb * ROWS, rlast = (r0 + ROWS < R ? r0 + ROWS : R) - 1;
    int nkeys = len - a.N + rlast / a.n_head + 1;
    nkeys = nkeys < 0 ? 0 : nkeys;
    const int ntiles = (nkeys + kMlaTile - 1) / kMlaTile;
    const int wr0 = r0 + wave * WR, wlast = (wr0 + WR < R ? wr0 + WR : R) - 1;
    const int wmin = wr0 < R ? len - a.N + wr0 / a.n_head : -1, wmax = wr0 < R ? len - a.N + wlast / a.n_head : -1;

    // ---- Q fragments, and the last key the lane's row attends ----
    const int r = wr0 + c;
    const bool live = r < R;
    const int tok = live ? r / a.n_head : 0, jh = live ? r - tok * a.n_head : 0;
    const int lim = live ? len - a.N + tok : -1;
    f16x8 qf[KS];
    {
        const uint16_t *q = a.Q + ((int64_t)b * a.N + tok) * a.ldq + (int64_t)jh * kMlaDk + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0, 0, 0, 0};
            if (live) v = ld16(q + 32 * ks);
            qf[ks] = __builtin_bit_cast(f16x8, v);
        }
    }

    // ---- the lane's 9 pieces of a tile's DMA (gguf_mla.hpp) ----
    const uint32_t span = (uint32_t)((int64_t)(a.capacity - 1) * a.tok_stride + kMlaRowB); // host: < 2^30
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(a.C + (int64_t)b * a.seq_stride), 0, (int)span, 0x00020000);
    int drow[NI];
    uint32_t doff[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) mla_dma_piece(k, tid, a.tok_stride, drow[k], doff[k]);
    auto issue = [&](int t) { // tile t into slot t % kMlaSlots; t >= ntiles: zeros, the same count
        uint8_t *dst = smem + (t % kMlaSlots) * kMlaTileB + 1024 * wave;
        const uint32_t tb = (uint32_t)t * kMlaTile * (uint32_t)a.tok_stride;
        uint32_t off[NI];
#pragma unroll
        for (int k = 0; k < NI; ++k) // no tile, a key no row of the block attends: outside the resource -- zeros, no access
            off[k] = t * kMlaTile + drow[k] < nkeys ? tb + doff[k] : 0x80000000u;
#pragma unroll
        for (int k = 0; k < NI; ++k) dma16(rs, dst + 4096 * k, off[k], 0);
    };

    float m = kNegInf, l = 0.f;
    f32x4 o[NG];
#pragma unroll
    for (int n = 0; n < NG; ++n) o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    uint32_t kbase[2], vbase[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) kbase[e] = mla_kbase(e, g, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) vbase[i] = mla_vbase(i, g, c);

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // Q has arrived: from here vmcnt counts DMAs only
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks])); // (used here: no wait for Q inside the loop)
#pragma unroll
    for (int s = 0; s < kMlaSlots - 1; ++s) issue(s);
    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI * (kMlaSlots - 2)) : "memory"); // this wave's pieces of tile t
        __syncthreads();                                                             // tile t has landed; tile t - 1's slot is drained
        issue(t + kMlaSlots - 1);
        const int key0 = t * kMlaTile;
        if (key0 <= wmax) { // (wave-uniform; otherwise the tile is wholly beyond this wave's rows)
            const uint32_t Ct = (t % kMlaSlots) * kMlaTileB;

            // ---- S^T = C Q^T, two 16-key tiles; k-steps 2j and 2j + 1 sit at kbase[0 / 1] + 128 j ----
            f32x4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < KS / 2; ++j) {
                f16x8 kf[2][2];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        kf[u][e] = __builtin_bit_cast(f16x8, *(const u32x4 *)(smem + Ct + kbase[e] + 16 * kMlaRowB * u + 128 * j));
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        s[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[u][e], qf[2 * j + e], s[u], 0, 0, 0);
            }
            // One wave per SIMD: nothing but the order of this wave's own instructions hides an LDS read's
            // latency (attn_mla.hip).  Six reads ahead, then one read per MFMA.
            __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
            for (int i = 0; i < 2 * KS - 6; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);

            // ---- online softmax in fp32 (a row's four lanes g hold 8 keys each) ----
            const bool crosses = key0 + kMlaTile - 1 > wmin; // some row of the wave ends inside this tile
            float sc[8], mx = kNegInf;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int key = key0 + (jj < 4 ? 4 * g + jj : 12 + 4 * g + jj); // the k-slot's key (attn_mla.hip)
                sc[jj] = s[jj >> 2][jj & 3] * a.c;
                if (crosses && key > lim) sc[jj] = kNegInf;
                mx = fmaxf(mx, sc[jj]);
            }
            mx = fmaxf(mx, xor_lanes(mx, 16));
            mx = fmaxf(mx, xor_lanes(mx, 32));
            const float mn = fmaxf(m, mx), mu = mn == kNegInf ? 0.f : mn;
            const float alpha = ex2(m - mu);
            float sum = 0.f;
            f16x8 pf;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const float p = ex2(sc[jj] - mu);
                sum += p; // the fp32 p, not the rounded operand
                pf[jj] = (_Float16)p;
            }
            l = l * alpha + sum;
            // the 128 accumulators are rescaled only when some row's maximum moved (wave-uniform; o is 0 while
            // m is -inf, so a skipped alpha of exp2(-inf - mu) = 0 scales nothing but zeros)
            if (__builtin_amdgcn_ballot_w64(mn != m && m != kNegInf)) {
#pragma unroll
                for (int n = 0; n < NG; ++n) o[n] *= alpha;
            }
            m = mn;

            // ---- O^T += C[:, :512]^T P^T: attn_mla.hip's transposing reads; column group n = 4 q + i sits
            // at vbase[i] + 128 q ----
#pragma unroll
            for (int q4 = 0; q4 < NG / 4; ++q4) {
                s16x4 half[4][2];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        half[i][u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (s16x4 __attribute__((address_space(3))) *)(smem + Ct + vbase[i] + 16 * kMlaRowB * u + 128 * q4));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f16x8 vf = __builtin_bit_cast(f16x8, __builtin_shufflevector(half[i][0], half[i][1], 0, 1, 2, 3, 4, 5, 6, 7));
                    o[4 * q4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[4 * q4 + i], 0, 0, 0);
                }
            }
            // (as above: eight 8-byte reads -- four MFMAs' worth -- ahead, then two reads per MFMA)
            __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
#pragma unroll
            for (int i = 0; i < NG - 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 1);
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the trailing (empty) tiles have landed

    // ---- a row's four lanes g hold its sum in parts and 4 of every 16 columns: o / l, rounded once ----
    float lt = l;
    lt += xor_lanes(lt, 16);
    lt += xor_lanes(lt, 32);
    if (!live) return;
    const float inv = lt > 0.f ? 1.0f / lt : 0.f; // (no key attended, the caller's kv_len < N: zeros)
    uint16_t *out = a.O + ((int64_t)b * a.N + tok) * a.ldo + (int64_t)jh * kMlaRank + 4 * g;
#pragma unroll
    for (int n = 0; n < NG; ++n) {
        const f32x4 v = o[n] * inv;
        const uint32_t lo = (uint32_t)f2h_bits(v[0]) | ((uint32_t)f2h_bits(v[1]) << 16);
        const uint32_t hi = (uint32_t)f2h_bits(v[2]) | ((uint32_t)f2h_bits(v[3]) << 16);
        if (a.o8) *(u32x2 *)(out + 16 * n) = (u32x2){lo, hi};
        else out[16 * n] = (uint16_t)lo, out[16 * n + 1] = (uint16_t)(lo >> 16), out[16 * n + 2] = (uint16_t)hi, out[16 * n + 3] = (uint16_t)(hi >> 16);
    }
}

} // namespace

MlaPrefillPlan plan_mla_prefill(int64_t B, int64_t N, int64_t n_head)
{
    MlaPrefillPlan p;
    if (B <= 0 || N <= 0 || n_head <= 0 || n_head > kMlaMaxHeads || B > (1 << 20) / 8) return p;
    if (N > INT32_MAX / (B * n_head)) return p; // B * N * n_head < 2^31
    p.nblk = (int)((N * n_head + kMlaPrefillRows - 1) / kMlaPrefillRows);
    p.grid = B * p.nblk;
    p.ok = true;
    return p;
}

hipError_t launch_mla_prefill(const MlaCall &c, const MlaPrefillPlan &p, hipStream_t s)
{
    MlaPrefillArgs a{};
    a.Q = (const uint16_t *)c.Q, a.C = (const uint8_t *)c.C, a.kv_len = c.kv_len, a.O = (uint16_t *)c.O;
    a.ldq = c.ldq, a.ldo = c.ldo, a.tok_stride = c.tok_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.n_head = (int)c.n_head, a.nblk = p.nblk, a.B = (int)c.B;
    a.o8 = (((uintptr_t)c.O | (uintptr_t)(2 * c.ldo)) & 7) == 0; // 8-byte stores of 4 columns
    a.c = c.scale * kLog2e;
    mla_prefill_kernel<<<dim3((unsigned)p.grid), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

} // namespace gq

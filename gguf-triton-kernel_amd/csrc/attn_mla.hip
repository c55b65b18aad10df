// attn_mla.hip -- DeepSeek's multi-head latent attention at decode, in its absorbed form, over an fp16
// latent cache (gq_mla_decode), its combine, and the cache's producer (gq_mla_append).  One shared
// "kv head" per sequence: a cache row is [c_kv (512) | k_pe (64)], the key is the whole row, the value
// its first 512 elements, and 16 .. 128 query heads of 1 .. 4 new tokens ride on that one row stream.
// The arithmetic, the kv_len semantics and the buffer-resource bounds are attn_decode.hip's; the work
// split is not.  No reference counterpart.
//
// Work split.  The R = N * n_head query rows (row r = token r / n_head, head r % n_head) are cut into
// groups of kMlaRows = 64; wave v of a workgroup's four owns the 16-row MFMA tile 16 v .. 16 v + 15 of
// its group for the whole kernel: its Q fragments (18 k-steps x 4 registers), its O^T accumulators
// (32 column groups x 4 fp32) and its online softmax never leave its registers.  Workgroup (b, group,
// w) of B * groups * W (W fixed on the host: plan_mla) takes the contiguous share [T w / W, T (w + 1)
// / W) of the sequence's T tiles of kMlaTile = 32 keys.  The four waves SHARE every tile (in
// attn_decode.hip each wave owns its tiles): 128 rows x 576 would not fit one wave, and a private K
// and V tile per wave at this width would not fit LDS.  A tile, 32 rows x 1152 bytes = 36 KiB, is
// loaded ONCE by LDS-DMA, every one of the 256 lanes issuing 9 16-byte pieces, and serves both
// products from the same bytes:
//   S^T[key 4g + i][row c] = sum_d C[key][d] Q[row][d]         18 k-steps, A = cache rows (ds_read_b128)
//   O^T[d 4g + i][row c]  += sum_key C[key][d] P[row][key]     32 groups of 16 columns d < 512, A = C^T
// with the keys in the A operand and k-slot 8g + j of the second product DEFINED as key (j < 4 ?
// 4g + j : 12 + 4g + j) as in the other two attention files; C^T comes from the transposing LDS read
// (ds_read_b64_tr_b16, two per 16 columns) attn_prefill.hip uses.  Waves own different rows, so nothing
// is merged across waves: each writes its tile's fp32 partial (m, l, o[16][512]) to the workspace and
// mla_combine_kernel merges a row's W partials in a fixed order and rounds to fp16 once.  No atomics, no
// workgroup waits for another.  A wave whose tile has no live row (n_head = 16, N = 1: one live tile
// of four) still issues its DMA quarter and meets the barriers; it skips its MFMAs and writes nothing
// (the combine reads live rows only).
//
// Ring.  kMlaSlots = 3 slots of one tile, 108 KiB of the 160: per tile i, s_waitcnt vmcnt(9) (the
// wave's pieces of tile i; those of tile i + 1 may still fly), ONE workgroup barrier (tile i has
// landed for everybody and everybody has finished tile i - 1), issue tile i + 2 into tile i - 1's
// slot, compute tile i.  Issues past the share go outside the buffer resource (zeros, no access), so
// the count the wait relies on is the same at the tail.  Two tiles, 72 KiB per compute unit, are in
// flight under the MFMAs: with one workgroup per compute unit (the ring and the 512-register budget
// both say so) nothing else hides the latency.  Reasoned, not measured against two slots.
// Resources (the compiler's report): 256 VGPRs + 140 AGPRs, no scratch, 110592 bytes of LDS.
//
// LDS rows and banks (reasoned, not measured).  A row is 72 16-byte pieces = 4.5 bank lines of 256
// bytes, so row r starts at bank-line offset 128 (r & 1) and unswizzled, one piece of 16 consecutive
// rows falls on two 16-byte bank columns only: an 8-way conflict.  Piece p of row r therefore sits at
// piece (p & ~7) | ((p & 7) ^ ((r >> 1) & 7)) -- the xor stays inside the row's aligned groups of 8
// pieces, 72 = 9 x 8, so it is a permutation of the row; the DMA picks the source piece per lane.  A
// piece's bank column is then (8 (r & 1) + (p & 8) + ((p & 7) ^ ((r >> 1) & 7))) mod 16: over 16
// consecutive rows (r & 1, (r >> 1) & 7) takes 16 distinct values, so the 16 lanes of a K-fragment
// read (16 rows, one piece) cover the 64 banks once, and the transposing read's 16 rows x 2 adjacent
// pieces (512 bytes) cover them twice, which is what 512 bytes cost anyway.
//
// Order of the workgroups.  With n_head = 128 two (N = 1) to eight (N = 4) row groups stream the same
// (b, w) share of the cache.  The hardware hands consecutive workgroup ids to the chip's kMlaXcd = 8
// dies in turn, each with its own L2, so the groups of one (b, w) are given ids 8 apart: id = 8 j + x
// is group j % groups of share (j / groups) * 8 + x, and one die meets a share's groups back to back.
// Ids past the last share (B * W no multiple of 8) exit at once.  Whether the second read then comes
// from L2 is a measurement, not a property of this order.
//
// Rows at or beyond the length and the issues past a share get a DMA offset outside the buffer
// resource: zeros, no access, so a dead row's bytes (NaN included) never reach an MFMA.  A live row
// beyond a query's own limit (N > 1) is masked to p = exactly 0.
//
// gq_mla_append (mla_append_kernel).  Workgroup (token, share) of 4 waves; a wave takes wave jobs:
// job 0 is the token's c_kv row -- lane l owns elements 8l .. 8l + 7, the sum of squares is a 64-lane
// butterfly, y = (x * rsqrt(mean + eps)) * w in fp32, rounded once into the cache row -- and job k > 0
// is two rotation jobs, one per half-wave of 32 pairs: rotation job 0 is k_pe into the cache row's
// last 64 elements, rotation job h + 1 is head h's q_pe into Qout's.  Lane l & 31 owns pair l & 31 in
// both modes, so its (m cos, m sin) (gguf_rope.hpp: rope.hip's fp64 angle) is formed once per token
// and kept over all the heads the wave walks.  No LDS, no scratch.
#include "gguf_attn.hpp"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"
#include "gguf_mla.hpp"
#include "gguf_rope.hpp"

namespace gq {
namespace {

// the tile geometry, the swizzle and the DMA and fragment addressing are gguf_mla.hpp's (shared with attn_mla_prefill.hip)
constexpr int kWaves = kMlaWaves;
constexpr int kRank = kMlaRank, kRope = kMlaRope, kDk = kMlaDk;
constexpr int kRowB = kMlaRowB, kNI = kMlaNI, kTileB = kMlaTileB, kKS = kMlaKS, kNG = kMlaNG;
constexpr int kMlaXcd = 8;                                 // dies that take workgroup ids in turn
constexpr float kNegInf = -__builtin_huge_valf();
typedef short s16x4 __attribute__((ext_vector_type(4)));
static_assert(kMlaRows == 16 * kWaves, "one 16-row MFMA tile per wave");

struct MlaArgs {
    const uint16_t *Q;
    const uint8_t *C;
    const int32_t *kv_len;
    uint16_t *O;
    float *ws;
    int64_t ldq, ldo, tok_stride, seq_stride;
    int capacity, N, n_head, W, groups, BW, o8;
    float c; // scale * log2(e): scores are kept in the exp2 domain
};

// floats of one workgroup's partial: o[64][512], then (m, l)[64]
constexpr int64_t kSlotF = (int64_t)kMlaRows * kRank + 2 * kMlaRows;

__global__ __launch_bounds__(256) void mla_decode_kernel(const MlaArgs a)
{
    __shared__ __attribute__((aligned(256))) uint8_t smem[kMlaSlots * kTileB];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // id = 8 j + x: group j % groups of share (j / groups) * 8 + x (the file header has the reason)
    const int x = (int)(blockIdx.x % (unsigned)kMlaXcd), j = (int)(blockIdx.x / (unsigned)kMlaXcd);
    const int grp = j % a.groups, bw = (j / a.groups) * kMlaXcd + x;
    if (bw >= a.BW) return;
    const int w = bw % a.W, b = bw / a.W;
    const int R = a.N * a.n_head;
    int len = a.kv_len[b];
    len = len < 0 ? 0 : (len > a.capacity ? a.capacity : len); // never outside the cache
    const int ntiles = (len + kMlaTile - 1) / kMlaTile;
    const int t0 = (int)((int64_t)ntiles * w / a.W), t1 = (int)((int64_t)ntiles * (w + 1) / a.W);
    float *part = a.ws + ((int64_t)bw * a.groups + grp) * kSlotF;
    const int r0 = grp * kMlaRows, wr0 = r0 + 16 * wave;
    if (t1 == t0) { // an empty share: the neutral partial (the combine skips its o)
        if (tid < kMlaRows && r0 + tid < R) *(f32x2 *)(part + kMlaRows * kRank + 2 * tid) = (f32x2){kNegInf, 0.f};
        return;
    }
    const bool wlive = wr0 < R; // (wave-uniform) some row of this wave's tile exists

    // ---- Q fragments, and the last key the lane's row attends ----
    const int r = wr0 + c;
    const bool live = r < R;
    const int tok = live ? r / a.n_head : 0, jh = live ? r - tok * a.n_head : 0;
    const int lim = live ? len - a.N + tok : -1;
    f16x8 qf[kKS];
    {
        const uint16_t *q = a.Q + ((int64_t)b * a.N + tok) * a.ldq + (int64_t)jh * kDk + 8 * g;
#pragma unroll
        for (int ks = 0; ks < kKS; ++ks) {
            u32x4 v = {0, 0, 0, 0};
            if (live) v = ld16(q + 32 * ks);
            qf[ks] = __builtin_bit_cast(f16x8, v);
        }
    }

    // ---- the lane's 9 pieces of a tile's DMA: LDS piece 256 k + tid <- (row, source piece) ----
    const uint32_t span = (uint32_t)((int64_t)(a.capacity - 1) * a.tok_stride + kRowB); // host: < 2^30
    const __amdgpu_buffer_rsrc_t rs =
        __builtin_amdgcn_make_buffer_rsrc((void *)(a.C + (int64_t)b * a.seq_stride), 0, (int)span, 0x00020000);
    int drow[kNI];
    uint32_t doff[kNI];
#pragma unroll
    for (int k = 0; k < kNI; ++k) mla_dma_piece(k, tid, a.tok_stride, drow[k], doff[k]);
    auto issue = [&](int t) { // tile t into slot (t - t0) % kMlaSlots; t >= t1: zeros, the same count
        uint8_t *dst = smem + ((t - t0) % kMlaSlots) * kTileB + 1024 * wave;
        const uint32_t tb = (uint32_t)t * kMlaTile * (uint32_t)a.tok_stride;
        uint32_t off[kNI];
#pragma unroll
        for (int k = 0; k < kNI; ++k) // no tile, a row at or beyond the length: outside the resource -- zeros, no access
            off[k] = t < t1 && t * kMlaTile + drow[k] < len ? tb + doff[k] : 0x80000000u;
#pragma unroll
        for (int k = 0; k < kNI; ++k) dma16(rs, dst + 4096 * k, off[k], 0);
    };

    float m = kNegInf, l = 0.f;
    f32x4 o[kNG];
#pragma unroll
    for (int n = 0; n < kNG; ++n) o[n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // key rows of the lane's 8 k-slots in the second product
    int vrow[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) vrow[jj] = jj < 4 ? 4 * g + jj : 12 + 4 * g + jj;

    // LDS offsets within a tile (gguf_mla.hpp): two bases serve the first product's 18 k-steps and four the
    // second's 32 column groups, everything else is an immediate offset
    uint32_t kbase[2], vbase[4];
#pragma unroll
    for (int e = 0; e < 2; ++e) kbase[e] = mla_kbase(e, g, c);
#pragma unroll
    for (int i = 0; i < 4; ++i) vbase[i] = mla_vbase(i, g, c);

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // Q has arrived: from here vmcnt counts DMAs only
#pragma unroll
    for (int ks = 0; ks < kKS; ++ks) asm volatile("" : "+v"(qf[ks])); // (used here: no wait for Q inside the loop)
#pragma unroll
    for (int s = 0; s < kMlaSlots - 1; ++s) issue(t0 + s);
    for (int t = t0; t < t1; ++t) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kNI * (kMlaSlots - 2)) : "memory"); // this wave's pieces of tile t
        __syncthreads();                                                               // tile t has landed; tile t - 1's slot is drained
        issue(t + kMlaSlots - 1);
        if (wlive) {
            const uint32_t Ct = ((t - t0) % kMlaSlots) * kTileB;
            const int key0 = t * kMlaTile;

            // ---- S^T = C Q^T, two 16-key tiles; k-steps 2j and 2j + 1 sit at kbase[0 / 1] + 128 j ----
            f32x4 s[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int j = 0; j < kKS / 2; ++j) {
                f16x8 kf[2][2];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int e = 0; e < 2; ++e)
                        kf[u][e] = __builtin_bit_cast(f16x8, *(const u32x4 *)(smem + Ct + kbase[e] + 16 * kRowB * u + 128 * j));
#pragma unroll
                for (int e = 0; e < 2; ++e)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        s[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[u][e], qf[2 * j + e], s[u], 0, 0, 0);
            }
            // One wave per SIMD: nothing but the order of this wave's own instructions hides an LDS read's latency,
            // and left alone the scheduler (200 registers live) puts every read right before its MFMA.  Six reads
            // ahead, then one read per MFMA.
            __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
            for (int i = 0; i < 2 * kKS - 6; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 6, 0);

            // ---- online softmax in fp32 (a row's four lanes g hold 8 keys each) ----
            float sc[8], mx = kNegInf;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                sc[jj] = key0 + vrow[jj] <= lim ? s[jj >> 2][jj & 3] * a.c : kNegInf;
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
                for (int n = 0; n < kNG; ++n) o[n] *= alpha;
            }
            m = mn;

            // ---- O^T += C[:, :512]^T P^T: lane c of group g sends rows 4g + c / 4 and 16 more, columns
            // 16n + 4 (c % 4) .. + 3, and receives column 16n + c of the group's four rows; column group
            // n = 4 q + i sits at vbase[i] + 128 q ----
#pragma unroll
            for (int q4 = 0; q4 < kNG / 4; ++q4) {
                s16x4 half[4][2];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int u = 0; u < 2; ++u)
                        half[i][u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                            (s16x4 __attribute__((address_space(3))) *)(smem + Ct + vbase[i] + 16 * kRowB * u + 128 * q4));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f16x8 vf = __builtin_bit_cast(f16x8, __builtin_shufflevector(half[i][0], half[i][1], 0, 1, 2, 3, 4, 5, 6, 7));
                    o[4 * q4 + i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, o[4 * q4 + i], 0, 0, 0);
                }
            }
            // (as above: eight 8-byte reads -- four MFMAs' worth -- ahead, then two reads per MFMA)
            __builtin_amdgcn_sched_group_barrier(0x100, 8, 1);
#pragma unroll
            for (int i = 0; i < kNG - 4; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 1);
                __builtin_amdgcn_sched_group_barrier(0x100, 2, 1);
            }
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 1);
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the trailing (empty) tiles have landed

    // ---- the wave's partial: a row's four lanes g hold its sum in parts and 4 of every 16 columns ----
    float lt = l;
    lt += xor_lanes(lt, 16);
    lt += xor_lanes(lt, 32);
    if (!live) return;
    const int lr = 16 * wave + c;
    if (g == 0) *(f32x2 *)(part + kMlaRows * kRank + 2 * lr) = (f32x2){m, lt};
#pragma unroll
    for (int n = 0; n < kNG; ++n) *(f32x4 *)(part + (int64_t)lr * kRank + 16 * n + 4 * g) = o[n];
}

// Row (b, r) of the output from its W partials.  With up to kMlaMaxW of them a serial walk is W dependent
// round trips to memory (measured: 100 us at W = 256), so the block is kCombWaves waves: wave v merges the
// partials w = v, v + 8, ... in that order with unconditional loads (lane l columns 8l .. 8l + 7; a neutral
// partial's never-written o is dropped by a select, not by a branch), then the waves' sums are added in wave
// order through LDS.  A fixed order for a given W: the bits depend on nothing else.
constexpr int kCombWaves = 8;
__global__ __launch_bounds__(64 * kCombWaves) void mla_combine_kernel(const MlaArgs a)
{
    __shared__ float mred[kCombWaves], lred[kCombWaves];
    __shared__ __attribute__((aligned(16))) float ored[kCombWaves][kRank];
    const int R = a.N * a.n_head;
    const int r = (int)(blockIdx.x % (unsigned)R), b = (int)(blockIdx.x / (unsigned)R);
    const int lane = threadIdx.x & 63, v = threadIdx.x >> 6;
    const int grp = r / kMlaRows, lr = r - grp * kMlaRows;
    const int64_t step = (int64_t)a.groups * kSlotF; // from w to w + 1
    const float *p0 = a.ws + ((int64_t)b * a.W * a.groups + grp) * kSlotF;
    const int ml = kMlaRows * kRank + 2 * lr;
    float mv = kNegInf;
#pragma unroll 4
    for (int w = v; w < a.W; w += kCombWaves) mv = fmaxf(mv, p0[w * step + ml]);
    if (lane == 0) mred[v] = mv;
    __syncthreads();
    float mm = kNegInf;
#pragma unroll
    for (int i = 0; i < kCombWaves; ++i) mm = fmaxf(mm, mred[i]);
    float lt = 0.f;
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int w = v; w < a.W; w += kCombWaves) {
        const float *p = p0 + w * step;
        const f32x2 st = *(const f32x2 *)(p + ml);
        const f32x4 x0 = *(const f32x4 *)(p + (int64_t)lr * kRank + 8 * lane), x1 = *(const f32x4 *)(p + (int64_t)lr * kRank + 8 * lane + 4);
        const bool dead = st.x == kNegInf; // a neutral partial: its o was never written, its l is 0
        const float f = dead ? 0.f : ex2(st.x - mm);
        lt += f * st.y;
        acc[0] += f * (dead ? zero : x0), acc[1] += f * (dead ? zero : x1);
    }
    if (lane == 0) lred[v] = lt;
    *(f32x4 *)&ored[v][8 * lane] = acc[0], *(f32x4 *)&ored[v][8 * lane + 4] = acc[1];
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= kRank / 4) return;
    float ls = 0.f;
    f32x4 sum = zero;
#pragma unroll
    for (int i = 0; i < kCombWaves; ++i) ls += lred[i], sum += *(const f32x4 *)&ored[i][4 * t];
    const int tok = r / a.n_head, jh = r - tok * a.n_head;
    uint16_t *out = a.O + ((int64_t)b * a.N + tok) * a.ldo + (int64_t)jh * kRank + 4 * t;
    const float inv = ls > 0.f ? 1.0f / ls : 0.f; // (no key attended, the caller's kv_len < N: zeros)
    const uint32_t lo = (uint32_t)f2h_bits(sum[0] * inv) | ((uint32_t)f2h_bits(sum[1] * inv) << 16);
    const uint32_t hi = (uint32_t)f2h_bits(sum[2] * inv) | ((uint32_t)f2h_bits(sum[3] * inv) << 16);
    if (a.o8) *(u32x2 *)out = (u32x2){lo, hi};
    else out[0] = (uint16_t)lo, out[1] = (uint16_t)(lo >> 16), out[2] = (uint16_t)hi, out[3] = (uint16_t)(hi >> 16);
}

struct MlaAppendArgs {
    const uint16_t *Ckv, *Kpe, *Qpe;
    uint16_t *Qo;
    uint8_t *C;
    const int32_t *kv_len;
    const float *inv_freq, *w;
    int64_t ldc, ldk, ldqp, qhs, ldqo, tok_stride, seq_stride;
    int capacity, N, n_head, passes, njobs;
    float mscale, eps;
    bool rows4, cache4, c16; // 4-byte accesses of the rotated pairs, 16-byte ones of the c_kv row
};

template <int MODE>
__global__ __launch_bounds__(256) void mla_append_kernel(const MlaAppendArgs a)
{
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int li = lane & 31, half = lane >> 5;
    const int64_t t = blockIdx.x;
    const int b = (int)(t / a.N), i = (int)(t - (int64_t)b * a.N);
    const int p = a.kv_len[b] - a.N + i;
    const bool inside = p >= 0 && p < a.capacity; // (outside: the caller's error, no cache row written)
    uint8_t *crow = a.C + (int64_t)b * a.seq_stride + (int64_t)p * a.tok_stride;
    const int e0 = MODE == 0 ? 2 * li : li, e1 = MODE == 0 ? 2 * li + 1 : li + kRope / 2;
    float cs = 0.f, sn = 0.f;
    bool have = false; // the angle: once per token and lane, at the first rotation job
    for (int k = 0; k < a.passes; ++k) {
        const int wj = ((int)blockIdx.y * a.passes + k) * kWaves + wave; // (wave-uniform)
        if (wj >= a.njobs) break;
        if (wj == 0) { // c_kv: the RMS norm of the 512, lane l elements 8l .. 8l + 7
            const uint16_t *src = a.Ckv + t * a.ldc + 8 * lane;
            uint16_t xin[8];
            if (a.c16) {
                const u32x4 v = *(const u32x4 *)src;
                __builtin_memcpy(xin, &v, 16);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) xin[e] = src[e];
            }
            float y[8], ss = 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) y[e] = h2f(xin[e]), ss = __builtin_fmaf(y[e], y[e], ss);
#pragma unroll
            for (int mk = 1; mk < 64; mk <<= 1) ss += __shfl_xor(ss, mk, 64);
            const float scale = 1.0f / sqrtf(ss * (1.0f / kRank) + a.eps);
            uint16_t out[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) out[e] = f2h_bits((y[e] * scale) * a.w[8 * lane + e]);
            if (inside) {
                uint16_t *dst = (uint16_t *)crow + 8 * lane;
                if (a.c16) {
                    u32x4 v;
                    __builtin_memcpy(&v, out, 16);
                    *(u32x4 *)dst = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) dst[e] = out[e];
                }
            }
            continue;
        }
        const int rj = 2 * (wj - 1) + half; // rotation job: 0 the token's k_pe, h + 1 head h's q_pe
        if (rj > a.n_head) continue;
        if (!have) rope_cs(p, a.inv_freq[li], a.mscale, cs, sn), have = true;
        const bool isk = rj == 0;
        const uint16_t *src = isk ? a.Kpe + t * a.ldk : a.Qpe + t * a.ldqp + (int64_t)(rj - 1) * a.qhs;
        const uint32_t in = load2(src, e0, e1, MODE == 0 && a.rows4);
        const float y0 = h2f(in & 0xffff), y1 = h2f(in >> 16);
        const uint32_t out = (uint32_t)f2h_bits(y0 * cs - y1 * sn) | ((uint32_t)f2h_bits(y0 * sn + y1 * cs) << 16);
        if (isk) {
            if (inside) store2((uint16_t *)crow + kRank, e0, e1, MODE == 0 && a.cache4, out);
        } else {
            store2(a.Qo + t * a.ldqo + (int64_t)(rj - 1) * kDk + kRank, e0, e1, MODE == 0 && a.rows4, out);
        }
    }
}

} // namespace

MlaPlan plan_mla(int64_t B, int64_t N, int64_t n_head)
{
    MlaPlan p;
    if (B <= 0 || N <= 0 || N > kMlaMaxN || n_head <= 0 || n_head > kMlaMaxHeads) return p;
    const int64_t groups = (N * n_head + kMlaRows - 1) / kMlaRows, BG = B * groups;
    if (BG > (1 << 20)) return p;
    p.ok = true;
    p.groups = (int)groups;
    // one workgroup per compute unit (the ring and the registers allow no second one), spread over the (b, group)
    const int64_t cus = num_cus(), pin = tuning().attn_w;
    const int64_t W = pin > 0 ? pin : (cus / BG < 1 ? 1 : (cus / BG > kMlaMaxW ? kMlaMaxW : cus / BG));
    p.W = (int)W;
    p.grid = (B * W + 7) / 8 * 8 * groups;
    // sized by a bound on BG * W that grows with B and the groups: min(kMlaMaxW BG, max(BG, cus))
    const int64_t slots = pin > 0 ? BG * W : (kMlaMaxW * BG < (BG > cus ? BG : cus) ? kMlaMaxW * BG : (BG > cus ? BG : cus));
    p.workspace_bytes = (size_t)(slots * kSlotF * 4);
    return p;
}

hipError_t launch_mla_decode(const MlaCall &c, const MlaPlan &p, hipStream_t s)
{
    MlaArgs a{};
    a.Q = (const uint16_t *)c.Q, a.C = (const uint8_t *)c.C, a.kv_len = c.kv_len, a.O = (uint16_t *)c.O, a.ws = (float *)c.workspace;
    a.ldq = c.ldq, a.ldo = c.ldo, a.tok_stride = c.tok_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.n_head = (int)c.n_head, a.W = p.W, a.groups = p.groups, a.BW = (int)(c.B * p.W);
    a.o8 = (((uintptr_t)c.O | (uintptr_t)(2 * c.ldo)) & 7) == 0; // 8-byte stores of 4 columns
    a.c = c.scale * kLog2e;
    mla_decode_kernel<<<dim3((unsigned)p.grid), dim3(256), 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    mla_combine_kernel<<<dim3((unsigned)(c.B * c.N * c.n_head)), dim3(64 * kCombWaves), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_mla_append(int mode, const MlaAppendCall &c, hipStream_t s)
{
    MlaAppendArgs a{};
    a.Ckv = (const uint16_t *)c.Ckv, a.Kpe = (const uint16_t *)c.Kpe, a.Qpe = (const uint16_t *)c.Qpe, a.Qo = (uint16_t *)c.Qout;
    a.C = (uint8_t *)c.C, a.kv_len = c.kv_len, a.inv_freq = c.inv_freq, a.w = c.norm_w;
    a.ldc = c.ldc, a.ldk = c.ldk, a.ldqp = c.ldqp, a.qhs = c.q_head_stride, a.ldqo = c.ldqo;
    a.tok_stride = c.tok_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.n_head = (int)c.n_head, a.mscale = c.mscale, a.eps = c.eps;
    const int64_t T = c.B * c.N;
    if (T == 0) return hipSuccess;
    a.rows4 = (((uintptr_t)c.Kpe | (uintptr_t)c.Qpe | (uintptr_t)c.Qout) & 3) == 0 && ((c.ldk | c.ldqp | c.q_head_stride | c.ldqo) & 1) == 0;
    a.cache4 = (((uintptr_t)c.C | (uintptr_t)c.tok_stride | (uintptr_t)c.seq_stride) & 3) == 0;
    a.c16 = (((uintptr_t)c.Ckv | (uintptr_t)(2 * c.ldc) | (uintptr_t)c.C | (uintptr_t)c.tok_stride | (uintptr_t)c.seq_stride) & 15) == 0;
    // wave jobs of a token: its c_kv row, then the n_head + 1 rotation jobs two by two; the shares of them
    // as rope.hip cuts its head jobs: as many as fill the chip twice over, at most one pass each
    a.njobs = 1 + (int)((c.n_head + 2) / 2);
    const int64_t ymax = (a.njobs + kWaves - 1) / kWaves, cus = num_cus(), want = (2 * cus + T - 1) / T;
    const int64_t Y = want < 1 ? 1 : (want > ymax ? ymax : want);
    a.passes = (int)((ymax + Y - 1) / Y);
    const dim3 grid((unsigned)T, (unsigned)((ymax + a.passes - 1) / a.passes)), block(256);
    if (mode == 0) mla_append_kernel<0><<<grid, block, 0, s>>>(a);
    else mla_append_kernel<1><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

} // namespace gq

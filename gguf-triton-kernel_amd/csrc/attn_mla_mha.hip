// attn_mla_mha.hip -- DeepSeek's multi-head latent attention over a prompt in its UN-absorbed form: the
// latent rows are decompressed once into per-head keys and values (gq_mla_kv_expand) and the new tokens
// attend at head dims 192 / 128 (gq_mla_prefill_mha) -- 2 (192 + 128) = 640 flops per attended (row, key)
// where the absorbed gq_mla_prefill pays 2 (576 + 512) = 2176.  The latent cache, its kv_len semantics and
// the append are attn_mla.hip's and are used unchanged.  No reference counterpart.
//
// ---- gq_mla_kv_expand -------------------------------------------------------------------------------
//
//   KV[b, p, h, m] = fp16( sum_c C[b, p, c] * W[h, m, c] )     m < 256, c < 512, p = kv_len[b] - N + i
//
// W (n_head, 256, 512): rows 0..127 of head h are k_b^T, rows 128..255 v_b, so the 256 values of (b, p, h)
// are [k_nope | v].  The mirror of mla_proj_tiled_kernel: there one head's W served one token tile's
// per-head X; here ONE X tile -- the c_kv of 64 or 128 positions of a sequence -- serves every head of a
// range.  A workgroup of four waves owns (sequence, token block, head range); wave v keeps the c_kv
// fragments of its RT = 1 or 2 16-token tiles in registers for the whole kernel (16 k-steps x 4 registers
// per tile), so c_kv is read from HBM once per (token block, head range).  D^T = W X^T as in
// attn_mla_proj.hip: the A operand is a 16-row tile of W, acc element i of lane (g, c) is KV[token c][m0 +
// 4 g + i], one 8-byte store.  The range's W is contiguous memory and is walked in 16 KiB stages (16 rows of
// 1024 bytes: one tile of W, 16 stages a head) through attn_mla_proj.hip's ring: three slots (48 KiB) filled by
// LDS-DMA, per stage s_waitcnt vmcnt(4) (this wave's four pieces of stage s; the stores of earlier stages
// only make the wait stricter -- loads return in order among themselves), ONE bare barrier, issue stage
// s + 2 into stage s - 1's slot, 16 RT MFMAs, RT stores.  Piece p of row r lands at piece p ^ (r & 15).
// Stage s of a range writes elements 16 s .. 16 s + 15 past the range's first head: the output of a (token,
// range) is one contiguous run.  With RT = 2 every W fragment read from LDS feeds two MFMAs, which is what
// balanced mla_proj_tiled_kernel's LDS-bound form on paper.  A position outside [0, min(capacity,
// kv_capacity)) and a token at or beyond N are zero fragments and are not stored.
// The split (plan_mla_kv_expand) follows from B, N, n_head and the number of compute units alone: 128-token
// blocks where that still leaves a workgroup per compute unit with every head its own range, else 64; then
// as many heads per range as leave two workgroups per compute unit.  Workgroups of one range are
// neighbours (id = range * blocks + block).
//
// ---- gq_mla_prefill_mha ------------------------------------------------------------------------------
//
//   o[b, i, h] = softmax_t( scale (q_nope . k_nope[b, t, h] + q_pe . k_pe[b, t]) ) v[b, t, h],  t <= kv_len[b] - N + i
//
// Work split.  MHA: a head's rows are its N tokens.  A workgroup of four waves owns ROWS = 64 or 128
// consecutive tokens of one (sequence, head); wave v owns RT = 1 or 2 16-row MFMA tiles -- its Q fragments
// (6 k-steps: 4 of q_nope, 2 of q_pe), its O^T accumulators (8 column groups) and its online softmax stay
// in its registers, 56 RT registers in all where mla_prefill_kernel holds 200 -- and finishes them alone:
// one launch, nothing split along the keys, no workspace.  ROWS = 128 where every compute unit still gets
// a workgroup (plan_mla_prefill_mha).  Workgroup ids count the row blocks from the last one down, and within
// a (row block, sequence) the heads: id = ((nblk - 1 - rb) B + b) n_head + h, so the workgroups that read the
// same k_pe bytes run next to each other.
//
// Ring.  A stage is kMhaTile = 64 keys: per key the head's 512 contiguous bytes [k_nope | v] of KV (32
// KiB) and the 128 bytes of k_pe from the latent cache row (8 KiB), 40 KiB, ten 16-byte LDS-DMA pieces per
// lane.  Two slots, 80 KiB: attn_prefill.hip's protocol (s_waitcnt vmcnt(0), ONE barrier, issue tile i + 1,
// compute tile i), and TWO workgroups per compute unit (160 KiB of LDS, at most 256 registers): the other
// workgroup's MFMAs run under this one's softmax and waits, which a third slot would not buy.
// LDS rows: [k_nope | v] rows are 512 bytes with piece p at (p & 16) | ((p & 15) ^ (r & 15)) -- each half is
// attn_prefill.hip's 256-byte row, whose bank argument holds unchanged because 512 = 0 mod 256 too -- and k_pe
// rows are 128 bytes with piece p at p ^ ((r >> 1) & 7), the D = 64 swizzle.
//
// Products per 32-key step, attn_prefill.hip's: S^T = K Q^T with keys in the A operand (k_nope's four
// k-steps, then k_pe's two, into the same accumulators), O^T += V^T P^T with V^T through the transposing
// LDS read and k-slot 8 g + j the key (j < 4 ? 4 g + j : 12 + 4 g + j).  fp32 scores in the exp2 domain, fp32
// softmax and sums, fp16 P, one final rounding.
//
// Causality is skipped, not masked: a workgroup fetches no key beyond its last row's position, a wave skips
// the steps wholly beyond its own last row, and the per-element compare runs only in steps that reach beyond
// the wave's first row.  Keys at or beyond the block's count get a DMA offset outside the buffer resource:
// zeros, no access, so dead bytes (NaN included) never reach an MFMA.
#include "gguf_attn.hpp"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"

namespace gq {
namespace {

constexpr float kNegInf = -__builtin_huge_valf();
typedef short s16x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x2 pack4(const f32x4 v)
{
    return (u32x2){(uint32_t)f2h_bits(v[0]) | ((uint32_t)f2h_bits(v[1]) << 16),
                   (uint32_t)f2h_bits(v[2]) | ((uint32_t)f2h_bits(v[3]) << 16)};
}

// ---------------------------------------------------------------------------------------------------
struct MlaExpandArgs {
    const uint16_t *W;
    const uint8_t *C;
    const int32_t *kv_len;
    uint8_t *KV;
    int64_t tok_stride, seq_stride, kv_tok_stride, kv_seq_stride;
    int lim, N, n_head, ntb, nbt, hpw; // lim = min(capacity, kv_capacity); nbt = B * ntb token blocks
};

constexpr int kExpKS = kMlaRank / 32;                          // 16 k-steps
constexpr int kExpStagesPerHead = kMlaKvWidth / 16;            // 16 stages of one 16-row tile of W
static_assert(16 * 2 * kMlaRank == kMlaProjStageB, "a stage is 16 rows of W: 16 KiB");

template <int RT>
__global__ __launch_bounds__(256) void mla_kv_expand_kernel(const MlaExpandArgs a)
{
    constexpr int NI = kMlaProjStageB / (16 * 256), PPR = kMlaRank / 8; // 4 DMAs per lane and stage, 64 pieces per row
    __shared__ __attribute__((aligned(256))) uint8_t smem[kMlaProjSlots * kMlaProjStageB];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int hr = blockIdx.x / (unsigned)a.nbt, bt = blockIdx.x % (unsigned)a.nbt;
    const int b = bt / a.ntb, tb = bt % a.ntb;
    const int h0 = hr * a.hpw, nh = a.n_head - h0 < a.hpw ? a.n_head - h0 : a.hpw;
    const int nst = nh * kExpStagesPerHead;
    const int len = a.kv_len[b];

    // ---- c_kv fragments of the wave's RT token tiles; a dead token is zeros and is not stored ----
    f16x8 xf[RT][kExpKS];
    bool live[RT];
    uint16_t *y[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int i = 64 * RT * tb + 16 * (RT * wave + rt) + c;
        const int64_t p = (int64_t)len - a.N + i;
        live[rt] = i < a.N && p >= 0 && p < a.lim;
        const int64_t pos = live[rt] ? p : 0;
        const uint8_t *x = a.C + (int64_t)b * a.seq_stride + pos * a.tok_stride + 16 * g;
#pragma unroll
        for (int s = 0; s < kExpKS; ++s) {
            u32x4 v = {0, 0, 0, 0};
            if (live[rt]) v = ld16(x + 64 * s);
            xf[rt][s] = __builtin_bit_cast(f16x8, v);
        }
        y[rt] = (uint16_t *)(a.KV + (int64_t)b * a.kv_seq_stride + pos * a.kv_tok_stride) + (int64_t)h0 * kMlaKvWidth + 4 * g;
    }

    // ---- the lane's NI pieces of a stage's DMA: LDS piece 256 k + tid <- piece pos ^ (row & 15) of its row ----
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.W + (int64_t)h0 * kMlaKvWidth * kMlaRank), 0, nst * kMlaProjStageB, 0x00020000); // <= 32 MiB
    uint32_t doff[NI];
#pragma unroll
    for (int k = 0; k < NI; ++k) {
        const int q = 256 * k + tid, r = q / PPR, pos = q % PPR;
        doff[k] = 16u * (uint32_t)(r * PPR + (pos ^ (r & 15)));
    }
    auto issue = [&](int st, int slot) { // st >= nst: outside the resource -- zeros, no access, the same count
        uint8_t *dst = smem + slot * kMlaProjStageB + 1024 * wave;
#pragma unroll
        for (int k = 0; k < NI; ++k)
            dma16(rs, dst + 4096 * k, st < nst ? (uint32_t)st * kMlaProjStageB + doff[k] : 0x80000000u, 0);
    };
    const uint32_t fbase = (uint32_t)(c * 2 * kMlaRank); // fragment s of a stage: row c, piece 4 s + g

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // c_kv has arrived: from here vmcnt counts DMAs (and KV's stores)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int s = 0; s < kExpKS; ++s) asm volatile("" : "+v"(xf[rt][s]));
    static_assert(kMlaProjSlots == 3, "the slot walk below");
    issue(0, 0);
    issue(1, 1);
    int slot = 0;
    for (int st = 0; st < nst; ++st) {
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory"); // this wave's pieces of stage st
        // (the bare barrier and the clobbers: mla_proj_tiled_kernel has the reason)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        issue(st + 2, slot == 0 ? 2 : slot - 1);
        const uint32_t S = slot * kMlaProjStageB + fbase;
        f32x4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < kExpKS; ++s) {
            const f16x8 wf = __builtin_bit_cast(f16x8, *(const u32x4 *)(smem + S + 16 * ((4 * s + g) ^ c)));
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf, xf[rt][s], acc[rt], 0, 0, 0);
        }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
            if (live[rt]) *(u32x2 *)(y[rt] + 16 * st) = pack4(acc[rt]);
        slot = slot == 2 ? 0 : slot + 1;
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the trailing (empty) stages have landed
}

// ---------------------------------------------------------------------------------------------------
struct MlaMhaArgs {
    const uint16_t *Qn, *Qp;
    const uint8_t *KV, *C;
    const int32_t *kv_len;
    uint16_t *O;
    int64_t ldqn, qnhs, ldqp, qphs, ldo, kv_tok_stride, kv_seq_stride, tok_stride, seq_stride;
    int capacity, lim, N, n_head, nblk, B; // lim = min(capacity, kv_capacity)
    float c;                               // scale * log2(e)
};

constexpr int kMhaKvRowB = 2 * kMlaKvWidth, kMhaPeRowB = 2 * kMlaRope;      // 512 and 128 bytes of a key in LDS
constexpr int kMhaKvB = kMhaTile * kMhaKvRowB, kMhaPeB = kMhaTile * kMhaPeRowB; // 32 KiB + 8 KiB
constexpr int kMhaSlotB = kMhaKvB + kMhaPeB;
constexpr int kMhaNIkv = kMhaKvB / (16 * 256), kMhaNIpe = kMhaPeB / (16 * 256); // 8 + 2 DMAs per lane and stage
constexpr int kMhaKSn = kMlaProjDim / 32, kMhaKSp = kMlaRope / 32, kMhaNG = kMlaProjDim / 16;

template <int RT>
__global__ __launch_bounds__(256, 2) void mla_prefill_mha_kernel(const MlaMhaArgs a)
{
    constexpr int WR = 16 * RT, ROWS = 4 * WR, KSN = kMhaKSn, KSP = kMhaKSp, KS = KSN + KSP, NG = kMhaNG, TK = kMhaTile;
    __shared__ __attribute__((aligned(256))) uint8_t smem[kMhaSlots * kMhaSlotB];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the last row block (the most keys) first; the heads of a (row block, sequence) neighbours
    const int h = (int)(blockIdx.x % (unsigned)a.n_head), rbb = (int)(blockIdx.x / (unsigned)a.n_head);
    const int rb = a.nblk - 1 - rbb / a.B, b = rbb % a.B;
    int len = a.kv_len[b];
    len = len < 0 ? 0 : (len > a.lim ? a.lim : len); // never outside the cache or the expanded buffer
    // keys the block's last row attends (0: none of its rows attends anything), and the wave's own limits
    const int r0 = rb * ROWS, rlast = (r0 + ROWS < a.N ? r0 + ROWS : a.N) - 1;
    int nkeys = len - a.N + rlast + 1;
    nkeys = nkeys < 0 ? 0 : nkeys;
    const int ntiles = (nkeys + TK - 1) / TK;
    const int wr0 = r0 + wave * WR, wlast = (wr0 + WR < a.N ? wr0 + WR : a.N) - 1;
    const int wmin = wr0 < a.N ? len - a.N + wr0 : -1, wmax = wr0 < a.N ? len - a.N + wlast : -1;

    // ---- Q fragments (k-steps 0..3 q_nope, 4..5 q_pe), and the last key each of the lane's rows attends ----
    f16x8 qf[RT][KS];
    int lim[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = wr0 + 16 * rt + c;
        const bool live = r < a.N;
        lim[rt] = live ? len - a.N + r : -1;
        const int64_t row = (int64_t)b * a.N + (live ? r : 0);
        const uint16_t *qn = a.Qn + row * a.ldqn + (int64_t)h * a.qnhs + 8 * g;
        const uint16_t *qp = a.Qp + row * a.ldqp + (int64_t)h * a.qphs + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0, 0, 0, 0};
            if (live) v = ld16(ks < KSN ? qn + 32 * ks : qp + 32 * (ks - KSN));
            qf[rt][ks] = __builtin_bit_cast(f16x8, v);
        }
    }

    // ---- the lane's pieces of a stage's DMA: LDS piece 256 k + tid of the part <- (key row, source piece) ----
    const uint32_t kvspan = (uint32_t)((int64_t)(a.lim - 1) * a.kv_tok_stride + kMhaKvRowB); // host: < 2^30
    const uint32_t pespan = (uint32_t)((int64_t)(a.capacity - 1) * a.tok_stride + kMhaPeRowB);
    const __amdgpu_buffer_rsrc_t kvrs = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.KV + (int64_t)b * a.kv_seq_stride + (int64_t)h * kMhaKvRowB), 0, (int)kvspan, 0x00020000);
    const __amdgpu_buffer_rsrc_t pers = __builtin_amdgcn_make_buffer_rsrc(
        (void *)(a.C + (int64_t)b * a.seq_stride + 2 * kMlaRank), 0, (int)pespan, 0x00020000);
    int kvrow[kMhaNIkv], perow[kMhaNIpe];
    uint32_t kvoff[kMhaNIkv], peoff[kMhaNIpe];
#pragma unroll
    for (int k = 0; k < kMhaNIkv; ++k) {
        const int q = 256 * k + tid, r = q >> 5, p = q & 31;
        kvrow[k] = r;
        kvoff[k] = (uint32_t)r * (uint32_t)a.kv_tok_stride + 16u * (uint32_t)((p & 16) | ((p & 15) ^ (r & 15)));
    }
#pragma unroll
    for (int k = 0; k < kMhaNIpe; ++k) {
        const int q = 256 * k + tid, r = q >> 3, p = q & 7;
        perow[k] = r;
        peoff[k] = (uint32_t)r * (uint32_t)a.tok_stride + 16u * (uint32_t)(p ^ f16_swz<64>(r));
    }
    auto issue = [&](int t) { // a key no row of the block attends: outside the resource -- zeros, no access
        uint8_t *dst = smem + (t % kMhaSlots) * kMhaSlotB + 1024 * wave;
        const uint32_t kvb = (uint32_t)t * TK * (uint32_t)a.kv_tok_stride, peb = (uint32_t)t * TK * (uint32_t)a.tok_stride;
#pragma unroll
        for (int k = 0; k < kMhaNIkv; ++k) dma16(kvrs, dst + 4096 * k, t * TK + kvrow[k] < nkeys ? kvb + kvoff[k] : 0x80000000u, 0);
#pragma unroll
        for (int k = 0; k < kMhaNIpe; ++k)
            dma16(pers, dst + kMhaKvB + 4096 * k, t * TK + perow[k] < nkeys ? peb + peoff[k] : 0x80000000u, 0);
    };

    float m[RT], l[RT];
    f32x4 o[RT][NG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        m[rt] = kNegInf, l[rt] = 0.f;
#pragma unroll
        for (int n = 0; n < NG; ++n) o[rt][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // LDS offsets within a 32-key step of the lane's reads.  K: row 16 u + c, piece (4 ks + g) ^ swizzle -- the
    // swizzle of rows c and 16 + c is the same.  V^T: rows 16 u + 4 g + c / 4, pieces 16 + ((2 n + (c >> 1 & 1)) ^ row).
    const uint32_t kn0 = (uint32_t)(c * kMhaKvRowB), kp0 = (uint32_t)(kMhaKvB + c * kMhaPeRowB);
    const int vr = 4 * g + (c >> 2);
    const uint32_t v0 = (uint32_t)(vr * kMhaKvRowB + 256 + 8 * (c & 1));

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // Q has arrived: from here vmcnt counts DMAs only
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[rt][ks]));
    if (ntiles > 0) issue(0);
    for (int t = 0; t < ntiles; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's share of tile t
        __syncthreads();                                  // tile t has landed; tile t - 1's slot is drained
        if (t + 1 < ntiles) issue(t + 1);
        const uint8_t *T0 = smem + (t % kMhaSlots) * kMhaSlotB;
#pragma unroll
        for (int st = 0; st < TK / 32; ++st) {
            const int key0 = t * TK + 32 * st;
            if (key0 > wmax) continue; // wholly beyond this wave's rows (wave-uniform)
            const uint8_t *Kn = T0 + 32 * st * kMhaKvRowB, *Kp = T0 + 32 * st * kMhaPeRowB;

            // ---- S^T = [K_nope | K_pe] Q^T, two 16-key tiles ----
            f32x4 s[2][RT];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) s[u][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) {
                    const uint8_t *at = ks < KSN ? Kn + kn0 + 16 * u * kMhaKvRowB + 16 * ((4 * ks + g) ^ c)
                                                 : Kp + kp0 + 16 * u * kMhaPeRowB + 16 * ((4 * (ks - KSN) + g) ^ f16_swz<64>(c));
                    const f16x8 kf = __builtin_bit_cast(f16x8, *(const u32x4 *)at);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) s[u][rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[rt][ks], s[u][rt], 0, 0, 0);
                }
            }

            // ---- online softmax in fp32, per row (a row's four lanes g hold 8 keys each) ----
            const bool crosses = key0 + 31 > wmin; // some row of the wave ends inside this step
            f16x8 pf[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float sc[8], mx = kNegInf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sc[j] = s[j >> 2][rt][j & 3] * a.c;
                    if (crosses && key0 + (j < 4 ? 4 * g + j : 12 + 4 * g + j) > lim[rt]) sc[j] = kNegInf;
                    mx = fmaxf(mx, sc[j]);
                }
                mx = fmaxf(mx, xor_lanes(mx, 16));
                mx = fmaxf(mx, xor_lanes(mx, 32));
                const float mn = fmaxf(m[rt], mx), mu = mn == kNegInf ? 0.f : mn;
                const float alpha = ex2(m[rt] - mu);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = ex2(sc[j] - mu);
                    sum += p; // the fp32 p, not the rounded operand
                    pf[rt][j] = (_Float16)p;
                }
                l[rt] = l[rt] * alpha + sum;
                m[rt] = mn;
#pragma unroll
                for (int n = 0; n < NG; ++n) o[rt][n] *= alpha;
            }

            // ---- O^T += V^T P^T: lane c of group g receives column 16 n + c of rows 4 g .. 4 g + 3 and 16 more ----
#pragma unroll
            for (int n = 0; n < NG; ++n) {
                s16x4 half[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) // (rows vr and 16 + vr share the swizzle)
                    half[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)(
                        Kn + v0 + 16 * u * kMhaKvRowB + 16 * ((2 * n + ((c >> 1) & 1)) ^ (vr & 15))));
                const f16x8 vf = __builtin_bit_cast(f16x8, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) o[rt][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[rt], o[rt][n], 0, 0, 0);
            }
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }

    // ---- a row's four lanes g hold its sum in parts and 4 of every 16 columns: o / l, rounded once ----
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float lt = l[rt];
        lt += xor_lanes(lt, 16);
        lt += xor_lanes(lt, 32);
        const float inv = lt > 0.f ? 1.0f / lt : 0.f; // (no key attended: zeros)
        const int r = wr0 + 16 * rt + c;
        if (r >= a.N) continue;
        uint16_t *out = a.O + ((int64_t)b * a.N + r) * a.ldo + (int64_t)h * kMlaProjDim + 4 * g;
#pragma unroll
        for (int n = 0; n < NG; ++n) *(u32x2 *)(out + 16 * n) = pack4(o[rt][n] * inv);
    }
}

} // namespace

MlaExpandPlan plan_mla_kv_expand(int64_t B, int64_t N, int64_t n_head)
{
    MlaExpandPlan p;
    if (B <= 0 || N <= 0 || n_head <= 0 || n_head > kMlaMaxHeads || B > (1 << 20) / 8 || N > INT32_MAX / B) return p;
    const int64_t cus = num_cus();
    p.rows = B * ((N + 127) / 128) * n_head >= cus ? 128 : 64;
    p.ntb = (int)((N + p.rows - 1) / p.rows);
    const int64_t blocks = B * p.ntb;
    int64_t ranges = (2 * cus + blocks - 1) / blocks; // two workgroups per compute unit where the heads allow
    ranges = ranges > n_head ? n_head : ranges;
    p.hpw = (int)((n_head + ranges - 1) / ranges);
    p.grid = blocks * ((n_head + p.hpw - 1) / p.hpw);
    p.ok = p.grid <= INT32_MAX;
    return p;
}

hipError_t launch_mla_kv_expand(const MlaMhaCall &c, const MlaExpandPlan &p, hipStream_t s)
{
    MlaExpandArgs a{};
    a.W = (const uint16_t *)c.W, a.C = (const uint8_t *)c.C, a.kv_len = c.kv_len, a.KV = (uint8_t *)c.KV;
    a.tok_stride = c.tok_stride, a.seq_stride = c.seq_stride, a.kv_tok_stride = c.kv_tok_stride, a.kv_seq_stride = c.kv_seq_stride;
    a.lim = (int)(c.capacity < c.kv_capacity ? c.capacity : c.kv_capacity);
    a.N = (int)c.N, a.n_head = (int)c.n_head, a.ntb = p.ntb, a.nbt = (int)(c.B * p.ntb), a.hpw = p.hpw;
    const dim3 grid((unsigned)p.grid), block(256);
    if (p.rows == 128) mla_kv_expand_kernel<2><<<grid, block, 0, s>>>(a);
    else mla_kv_expand_kernel<1><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

MlaMhaPlan plan_mla_prefill_mha(int64_t B, int64_t N, int64_t n_head)
{
    MlaMhaPlan p;
    if (B <= 0 || N <= 0 || n_head <= 0 || n_head > kMlaMaxHeads || B > (1 << 20) / 8) return p;
    if (N > INT32_MAX / (B * n_head)) return p; // B * N * n_head < 2^31
    // 128 rows where every compute unit still gets a workgroup, 64 otherwise
    p.rows = B * n_head * ((N + 127) / 128) >= num_cus() ? 128 : 64;
    p.nblk = (int)((N + p.rows - 1) / p.rows);
    p.grid = B * n_head * p.nblk;
    p.ok = true;
    return p;
}

hipError_t launch_mla_prefill_mha(const MlaMhaCall &c, const MlaMhaPlan &p, hipStream_t s)
{
    MlaMhaArgs a{};
    a.Qn = (const uint16_t *)c.Qn, a.Qp = (const uint16_t *)c.Qp, a.KV = (const uint8_t *)c.KV, a.C = (const uint8_t *)c.C;
    a.kv_len = c.kv_len, a.O = (uint16_t *)c.O;
    a.ldqn = c.ldqn, a.qnhs = c.qn_head_stride, a.ldqp = c.ldqp, a.qphs = c.qp_head_stride, a.ldo = c.ldo;
    a.kv_tok_stride = c.kv_tok_stride, a.kv_seq_stride = c.kv_seq_stride, a.tok_stride = c.tok_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.lim = (int)(c.capacity < c.kv_capacity ? c.capacity : c.kv_capacity);
    a.N = (int)c.N, a.n_head = (int)c.n_head, a.nblk = p.nblk, a.B = (int)c.B;
    a.c = c.scale * kLog2e;
    const dim3 grid((unsigned)p.grid), block(256);
    if (p.rows == 128) mla_prefill_mha_kernel<2><<<grid, block, 0, s>>>(a);
    else mla_prefill_mha_kernel<1><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

} // namespace gq

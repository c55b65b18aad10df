// attn_decode.hip -- causal softmax attention of 1..4 new tokens per sequence over an fp16 or Q8_0
// KV cache with grouped query heads (gq_attn_decode), its combine, and the cache's device-side
// producer (gq_kv_append).  No reference counterpart.
//
// Work split.  Workgroup (b, h, w) of B * n_kv_head * W (W fixed on the host: plan_attn) reads
// kv_len[b], cuts the sequence into tiles of kAttnTile keys and takes the contiguous share
// [T w / W, T (w + 1) / W) of the T tiles; inside it wave v of 4 takes every fourth tile.  A wave
// never waits for another one before the end: it owns a ring of kAttnRing slots in LDS, each a K
// tile and a V tile, filled by LDS-DMA (dma16) and waited for by counted vmcnt -- tile i + 1 is in
// flight under tile i's MFMAs, and the V tile is still in flight under QK^T.
//
// All R = N * G query rows of the kv head (row r = token r / G, head h G + r % G) ride together as
// one or two 16-row tiles (RT), their Q fragments in registers for the whole kernel.  Both products
// put the key side in the A operand of v_mfma_f32_16x16x32_f16, so that a lane's query row is its
// column l & 15 in both accumulators and the online softmax needs no transposition:
//   S^T[key 4g + i][row c] = sum_d K[key][d] Q[row][d]     A = K rows (d contiguous), B = Q
//   O^T[d 4g + i][row c]  += sum_key V[key][d] P[row][key]  A = V^T (gathered), B = P
// (g = l >> 4, c = l & 15).  The two S^T tiles of a 32-key tile leave lane (g, c) with row c's scores
// of keys 4g + i and 16 + 4g + i: exactly the 8 k-slots 8g + j of the second product once slot
// 8g + j is DEFINED as key (j < 4 ? 4g + j : 12 + 4g + j); the V^T fragment gathers the same keys.
//
// LDS layout.  fp16: a tile is 32 rows of D/8 16-byte pieces; piece p of row r sits at piece
// p ^ (r & 15) (D = 128) or p ^ ((r >> 1) & 7) (D = 64) -- the DMA picks the source piece per lane.
// With it the 16 lanes of a K fragment read (16 rows, one piece) cover all 64 banks once, and the
// 64 lanes of a V^T gather (2 bytes each: 4 key rows x 16 columns) touch 32 distinct banks.
// Q8_0: a row is its D/32 34-byte blocks moved as raw bytes from a 2-byte aligned source into
// ceil(34 D / 512) pieces (144 / 80 bytes per row); codes are read as aligned dwords and shifted.
// Rows at or beyond the length are never fetched: their DMA offset lies outside the buffer
// resource, which writes zeros, so a dead row's bytes (NaN included) never reach an MFMA.
//
// Q8_0 arithmetic.  Codes are widened to exact fp16 (1024 + (code ^ 0x80) - 1152).  K: one block is
// one MFMA k-step from a zero accumulator, then s += d_block * partial in fp32.  V: the token's block
// scale is folded into P, fp16(p * d) per 32 output columns.  No weight is rounded.
//
// Each workgroup merges its four waves through LDS and writes one fp32 partial (m, l, o[R][D]) to
// the workspace; attn_combine_kernel merges the W partials of a row in w order.  No atomics, no
// workgroup waits for another.
//
// D = 256 (Gemma).  Two slots per wave would be 4 x 2 x 32 KiB at fp16 against 160 KiB of LDS, so a
// wave keeps ONE slot and refills it by halves: the K half as soon as QK^T has read it (in flight
// under the softmax and the second product of the same tile), the V half after the second product
// (in flight under the next tile's QK^T).  Half a tile per wave, 64 KiB per compute unit at fp16, is
// always on its way under MFMAs; the slot's LDS reads are drained (lgkmcnt(0)) before the DMA that
// overwrites it is issued.  Ring 4 x 32 KiB = 128 KiB (Q8_0: 4 x 18 KiB); the merge area,
// 4 * ROWS * (D + 2) * 4 = 129 KiB at two row tiles, overlays it.  fp16 rows are 512 bytes = 32
// pieces, piece p of row r at p ^ (r & 15): a row is two bank lines, the xor moves the piece within
// its line, so the 16 rows of a K fragment read still cover the 64 banks once.  fp16 V^T comes from
// prefill's two transposing reads (ds_read_b64_tr_b16) per 16 columns, not from eight 2-byte gathers:
// with the gather the two-row-tile kernel spilled to scratch.  The DMA geometry is recomputed per
// issue (2 x 16 registers otherwise live across the loop).
//
// Sliding window (gq_attn_opts.window > 0): row of position p attends [max(0, p - window + 1), p].
// The tile range is cut, not only masked: the W workgroups share the tiles from the one that holds
// the FIRST row's window start to the last row's limit, rows before that start are not fetched, and
// the per-row lower bound is one more compare on the key index.  A masked score is -inf, its p an
// exact 0, so a fetched key outside a row's window adds 0 * (finite) = 0.
//
// Soft-cap (gq_attn_opts.softcap > 0; the CAP instantiations -- the others keep their code): the
// score becomes cap * tanh(scale s / cap), in the exp2 domain cc * tanh(x) with cc = cap log2(e),
// x = s * scale / cap, and tanh(x) = 1 - 2 / (1 + 2^(2 log2(e) x)): one v_exp_f32, one v_rcp_f32,
// one fma, saturating to +-1 through inf and 0 without a branch.  Absolute error of the tanh below
// 2^-21, i.e. cap * 2^-21 in the exponent: 2^-15 at cap 50.
#include "gguf_attn.hpp"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"
#include "quant/gguf_quant_blocks.hpp"

namespace gq {
namespace {

constexpr int kAttnWaves = 4;
constexpr float kNegInf = -__builtin_huge_valf();
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct AttnArgs {
    const uint16_t *Q;
    const uint8_t *Kc, *Vc;
    const int32_t *kv_len;
    uint16_t *O;
    float *ws;
    int64_t ldq, ldo, tok_stride, head_stride, seq_stride;
    int capacity, N, G, n_kv, W;
    int window;   // 0: unbounded
    float c;      // scale * log2(e): scores are kept in the exp2 domain
    float cx, cc; // soft-cap: 2 log2(e) scale / cap and cap log2(e)
};

// floats per partial slot: o[R][D], then (m, l)[R], padded to 16 bytes
__host__ __device__ constexpr int64_t attn_slot_floats(int64_t R, int64_t D) { return R * D + ((2 * R + 3) & ~(int64_t)3); }

template <int KV, int D> struct ATile {
    static constexpr int RB = KV ? 34 * (D / 32) : 2 * D;        // bytes of a cache row
    static constexpr int PPR = (RB + 15) / 16;                   // 16-byte pieces per LDS row
    static constexpr int ROWB = 16 * PPR;
    static constexpr int NI = (kAttnTile * PPR + 63) / 64;       // DMA instructions per K (or V) tile
    static constexpr int TILEB = 1024 * NI;
    static constexpr int SLOT = 2 * TILEB;                       // K tile, V tile
    static constexpr int SLOTS = D == 256 ? 1 : kAttnRing;       // D = 256: one slot, refilled by halves
    static constexpr int RING = kAttnWaves * SLOTS * SLOT;
};

template <int KV, int D, int RT, bool CAP>
__global__ __launch_bounds__(256) void attn_decode_kernel(const AttnArgs a)
{
    using T = ATile<KV, D>;
    constexpr int ROWS = 16 * RT, NI = T::NI, KS = D / 32, NG = D / 16;
    constexpr bool HALVES = T::SLOTS == 1;
    constexpr int MERGE = kAttnWaves * ROWS * (D + 2) * 4;
    __shared__ __attribute__((aligned(16))) uint8_t smem[T::RING > MERGE ? T::RING : MERGE];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int w = (int)(blockIdx.x % (unsigned)a.W), bh = (int)(blockIdx.x / (unsigned)a.W);
    const int h = bh % a.n_kv, b = bh / a.n_kv;
    const int R = a.N * a.G;
    int len = a.kv_len[b];
    len = len < 0 ? 0 : (len > a.capacity ? a.capacity : len); // never outside the cache
    // the first row's window start (0 without a window): no tile and no row before it is fetched
    const int wlo = a.window > 0 && len - a.N - a.window + 1 > 0 ? len - a.N - a.window + 1 : 0;
    const int tlo = wlo / kAttnTile, ntiles = (len + kAttnTile - 1) / kAttnTile - tlo;
    const int t0 = tlo + (int)((int64_t)ntiles * w / a.W), t1 = tlo + (int)((int64_t)ntiles * (w + 1) / a.W);
    float *part = a.ws + (int64_t)blockIdx.x * attn_slot_floats(R, D);
    if (t1 == t0) { // an empty share: the neutral partial (the combine skips its o)
        if (tid < R) *(f32x2 *)(part + (int64_t)R * D + 2 * tid) = (f32x2){kNegInf, 0.f};
        return;
    }
    const int ntile = t1 - t0 > wave ? (t1 - t0 - wave + kAttnWaves - 1) / kAttnWaves : 0; // this wave's

    // ---- Q fragments, and the last key each of the lane's rows attends ----
    f16x8 qf[RT][KS];
    int lim[RT], lo[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = 16 * rt + c;
        const bool live = r < R;
        const int tok = live ? r / a.G : 0, jh = live ? r - tok * a.G : 0;
        lim[rt] = live ? len - a.N + tok : -1;
        lo[rt] = a.window > 0 ? lim[rt] - a.window + 1 : 0; // (negative: no lower bound)
        const uint16_t *q = a.Q + ((int64_t)b * a.N + tok) * a.ldq + ((int64_t)h * a.G + jh) * D + 8 * g;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            u32x4 v = {0, 0, 0, 0};
            if (live) v = ld16(q + 32 * ks);
            const f16x8 f = __builtin_bit_cast(f16x8, v);
            // Q8_0: the widened codes come in the element order (0,2,1,3,4,6,5,7) (pair02 / pair13)
            qf[rt][ks] = KV ? __builtin_shufflevector(f, f, 0, 2, 1, 3, 4, 6, 5, 7) : f;
        }
    }

    // ---- the DMA's per-lane geometry: LDS piece 64k + lane of a tile <- (row, source piece) ----
    const uint32_t span = (uint32_t)((int64_t)(a.capacity - 1) * a.tok_stride + T::RB); // host: < 2^31
    const int64_t base = (int64_t)b * a.seq_stride + (int64_t)h * a.head_stride;
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.Kc + base), 0, (int)span, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.Vc + base), 0, (int)span, 0x00020000);
    auto geom = [&](int ln, int k, int &row, uint32_t &at) {
        const int s = 64 * k + ln, r = s / T::PPR, p = s - r * T::PPR;
        row = r < kAttnTile ? r : 0x40000000; // (Q8_0: the last instruction's spare lanes fetch nothing)
        at = (uint32_t)(r & (kAttnTile - 1)) * (uint32_t)a.tok_stride + 16u * (uint32_t)(KV ? p : (p ^ f16_swz<D>(r)));
    };
    // D = 256: 2 x 16 registers of geometry would not fit beside the accumulators -- recomputed per issue instead
    int drow[HALVES ? 1 : NI];
    uint32_t doff[HALVES ? 1 : NI];
    if constexpr (!HALVES) {
#pragma unroll
        for (int k = 0; k < NI; ++k) geom(lane, k, drow[k], doff[k]);
    }
    uint8_t *ring = smem + wave * (T::SLOTS * T::SLOT);
    // which: 1 the K tile, 2 the V tile, 3 both
    auto issue = [&](int i, int which) {
        const int t = t0 + wave + kAttnWaves * i;
        const bool real = i < ntile;
        uint8_t *dst = ring + (i % T::SLOTS) * T::SLOT;
        const uint32_t tb = (uint32_t)t * kAttnTile * (uint32_t)a.tok_stride;
        uint32_t off[NI];
        int ln = lane;
        if constexpr (HALVES) asm volatile("" : "+v"(ln)); // (opaque: keeps the geometry out of the loop's live registers)
#pragma unroll
        for (int k = 0; k < NI; ++k) { // no tile, a spare lane, a dead row, a row before the window: outside the resource -- zeros, no access
            int row = drow[HALVES ? 0 : k];
            uint32_t at = doff[HALVES ? 0 : k];
            if constexpr (HALVES) geom(ln, k, row, at);
            const int key = t * kAttnTile + row;
            off[k] = real && key < len && key >= wlo ? tb + at : 0x80000000u;
        }
        if (which & 1) {
#pragma unroll
            for (int k = 0; k < NI; ++k) dma16(krs, dst + 1024 * k, off[k], 0);
        }
        if (which & 2) {
#pragma unroll
            for (int k = 0; k < NI; ++k) dma16(vrs, dst + T::TILEB + 1024 * k, off[k], 0);
        }
    };

    float m[RT], l[RT];
    f32x4 o[RT][NG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        m[rt] = kNegInf, l[rt] = 0.f;
#pragma unroll
        for (int n = 0; n < NG; ++n) o[rt][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // key rows of the lane's 8 k-slots in the second product
    int vrow[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) vrow[j] = j < 4 ? 4 * g + j : 12 + 4 * g + j;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // Q has arrived: from here vmcnt counts DMAs only
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[rt][ks])); // (used here: no wait for Q inside the loop)
    issue(0, 3);
    for (int i = 0; i < ntile; ++i) {
        if constexpr (!HALVES) issue(i + 1, 3); // (past the last tile: zeros, the same count)
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HALVES ? NI : 3 * NI) : "memory"); // tile i's K
        const uint8_t *Kt = ring + (i % T::SLOTS) * T::SLOT, *Vt = Kt + T::TILEB;
        const int key0 = (t0 + wave + kAttnWaves * i) * kAttnTile;

        // ---- S^T = K Q^T, two 16-key tiles ----
        f32x4 s[2][RT];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int r = 16 * u + c;
            const uint8_t *row = Kt + r * T::ROWB;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) s[u][rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                if constexpr (KV == 0) {
                    const f16x8 kf = __builtin_bit_cast(f16x8, *(const u32x4 *)(row + 16 * ((4 * ks + g) ^ f16_swz<D>(r))));
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        s[u][rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[rt][ks], s[u][rt], 0, 0, 0);
                } else {
                    // the lane's 8 codes start 0 or 2 bytes past a dword (the same for the whole k-step)
                    const int off = 34 * ks + 2 + 8 * g, sh = (34 * ks + 2) & 3;
                    const uint32_t *al = (const uint32_t *)(row + (off & ~3));
                    const uint32_t w0 = al[0], w1 = al[1];
                    u32x2 q = {w0, w1};
                    if (sh) q = (u32x2){__builtin_amdgcn_alignbyte(w1, w0, 2), __builtin_amdgcn_alignbyte(al[2], w1, 2)};
                    const uint32_t c0 = q.x ^ 0x80808080u, c1 = q.y ^ 0x80808080u;
                    const h2 bias = splat(-1152.f);
                    const f16x8 kf = frag4(pair02(c0) + bias, pair13(c0) + bias, pair02(c1) + bias, pair13(c1) + bias);
                    float dk[4]; // block scales of the accumulator's keys 16u + 4g + i
#pragma unroll
                    for (int e = 0; e < 4; ++e) dk[e] = h2f(*(const uint16_t *)(Kt + (16 * u + 4 * g + e) * T::ROWB + 34 * ks));
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                        const f32x4 pr = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf[rt][ks], z, 0, 0, 0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) s[u][rt][e] = __builtin_fmaf(dk[e], pr[e], s[u][rt][e]);
                    }
                }
            }
        }

        if constexpr (HALVES) { // the K half is read: tile i + 1's K goes into it, under the softmax and the second product
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(i + 1, 1);
        }

        // ---- online softmax in fp32, per row (a row's four lanes g hold 8 keys each) ----
        f16x8 pf[RT];
        float p[RT][8];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            float sc[8], mx = kNegInf;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int key = key0 + vrow[j];
                const float sv = s[j >> 2][rt][j & 3];
                sc[j] = key <= lim[rt] && key >= lo[rt] ? (CAP ? capped(sv * a.cx, a.cc) : sv * a.c) : kNegInf;
                mx = fmaxf(mx, sc[j]);
            }
            mx = fmaxf(mx, xor_lanes(mx, 16));
            mx = fmaxf(mx, xor_lanes(mx, 32));
            const float mn = fmaxf(m[rt], mx), mu = mn == kNegInf ? 0.f : mn;
            const float alpha = ex2(m[rt] - mu);
            float sum = 0.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                p[rt][j] = ex2(sc[j] - mu);
                sum += p[rt][j]; // the fp32 p, not the rounded operand
            }
            l[rt] = l[rt] * alpha + sum;
            m[rt] = mn;
#pragma unroll
            for (int n = 0; n < NG; ++n) o[rt][n] *= alpha;
            if constexpr (KV == 0) {
#pragma unroll
                for (int j = 0; j < 8; ++j) pf[rt][j] = (_Float16)p[rt][j];
            }
        }

        // ---- O^T += V^T P^T ----
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(HALVES ? NI : 2 * NI) : "memory"); // tile i's V
        if constexpr (KV == 0) {
#pragma unroll
            for (int n = 0; n < NG; ++n) {
                f16x8 vf;
                if constexpr (D == 256) {
                    // two transposing reads (ds_read_b64_tr_b16), as prefill's: lane c of group g sends rows 4g + c / 4
                    // and 16 more, columns 16n + 4 (c % 4) .. + 3, and receives column 16n + c of the group's four rows
                    s16x4 half[2];
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int r = 16 * u + 4 * g + (c >> 2);
                        const uint8_t *at = Vt + r * T::ROWB + 16 * ((2 * n + ((c >> 1) & 1)) ^ f16_swz<D>(r)) + 8 * (c & 1);
                        half[u] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((s16x4 __attribute__((address_space(3))) *)at);
                    }
                    vf = __builtin_bit_cast(f16x8, __builtin_shufflevector(half[0], half[1], 0, 1, 2, 3, 4, 5, 6, 7));
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const int r = vrow[j];
                        vf[j] = *(const _Float16 *)(Vt + r * T::ROWB + 16 * ((2 * n + (c >> 3)) ^ f16_swz<D>(r)) + 2 * (c & 7));
                    }
                }
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) o[rt][n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[rt], o[rt][n], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int bn = 0; bn < KS; ++bn) {
                // the token's block scale folded into P for this block's 32 output columns
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        pf[rt][j] = (_Float16)(p[rt][j] * h2f(*(const uint16_t *)(Vt + vrow[j] * T::ROWB + 34 * bn)));
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    const uint8_t *col = Vt + 34 * bn + 2 + 16 * hf + c;
                    h2 v2[4];
#pragma unroll
                    for (int j = 0; j < 8; j += 2) {
                        const uint32_t lo = col[vrow[j] * T::ROWB], hi = col[vrow[j + 1] * T::ROWB];
                        v2[j >> 1] = as_h2((lo | (hi << 16)) ^ 0x64806480u) + splat(-1152.f);
                    }
                    const f16x8 vf = frag4(v2[0], v2[1], v2[2], v2[3]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
                        o[rt][2 * bn + hf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[rt], o[rt][2 * bn + hf], 0, 0, 0);
                }
            }
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the next issue into it
        if constexpr (HALVES) { // the V half is read: tile i + 1's V goes into it, under the next QK^T
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            issue(i + 1, 2);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the trailing (empty) tile has landed: the ring is dead
    __syncthreads();

    // ---- the four waves' states through LDS, merged in wave order, one partial per workgroup ----
    float *mb = (float *)smem, *lb = mb + kAttnWaves * ROWS, *ob = lb + kAttnWaves * ROWS;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float lt = l[rt];
        lt += xor_lanes(lt, 16);
        lt += xor_lanes(lt, 32);
        const int r = 16 * rt + c;
        if (g == 0) mb[wave * ROWS + r] = m[rt], lb[wave * ROWS + r] = lt;
#pragma unroll
        for (int n = 0; n < NG; ++n) *(f32x4 *)(ob + ((int64_t)(wave * ROWS + r) * D + 16 * n + 4 * g)) = o[rt][n];
    }
    __syncthreads();
    for (int idx = tid; idx < R * (D / 4); idx += 256) {
        const int r = idx / (D / 4), d4 = idx - r * (D / 4);
        float mm = kNegInf;
#pragma unroll
        for (int v = 0; v < kAttnWaves; ++v) mm = fmaxf(mm, mb[v * ROWS + r]);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        float lt = 0.f;
        if (mm != kNegInf) {
#pragma unroll
            for (int v = 0; v < kAttnWaves; ++v) {
                const float f = ex2(mb[v * ROWS + r] - mm);
                lt += f * lb[v * ROWS + r];
                acc += f * *(const f32x4 *)(ob + ((int64_t)(v * ROWS + r) * D + 4 * d4));
            }
        }
        *(f32x4 *)(part + (int64_t)r * D + 4 * d4) = acc;
        if (d4 == 0) *(f32x2 *)(part + (int64_t)R * D + 2 * r) = (f32x2){mm, lt};
    }
}

// Row (b, h, r) of the output from its W partials, in w order: block = one row (64 threads, 128 at D = 256),
// thread t columns 2t, 2t + 1
template <int D>
__global__ __launch_bounds__(D > 128 ? D / 2 : 64) void attn_combine_kernel(const AttnArgs a)
{
    const int R = a.N * a.G;
    const int r = (int)(blockIdx.x % (unsigned)R), bh = (int)(blockIdx.x / (unsigned)R);
    const int h = bh % a.n_kv, b = bh / a.n_kv, t = threadIdx.x;
    if (2 * t >= D) return;
    const int64_t sf = attn_slot_floats(R, D);
    const float *p0 = a.ws + (int64_t)bh * a.W * sf;
    float mm = kNegInf;
    for (int w = 0; w < a.W; ++w) mm = fmaxf(mm, p0[w * sf + (int64_t)R * D + 2 * r]);
    float lt = 0.f, x = 0.f, y = 0.f;
    for (int w = 0; w < a.W; ++w) {
        const float *p = p0 + w * sf;
        const float mw = p[(int64_t)R * D + 2 * r];
        if (mw == kNegInf) continue; // a neutral partial: its o was never written
        const float f = ex2(mw - mm);
        lt += f * p[(int64_t)R * D + 2 * r + 1];
        const f32x2 v = *(const f32x2 *)(p + (int64_t)r * D + 2 * t);
        x += f * v.x, y += f * v.y;
    }
    const int tok = r / a.G, jh = r - tok * a.G;
    uint16_t *out = a.O + ((int64_t)b * a.N + tok) * a.ldo + ((int64_t)h * a.G + jh) * D + 2 * t;
    out[0] = lt > 0.f ? f2h_bits(x / lt) : (uint16_t)0; // (no key attended: the caller's kv_len < N)
    out[1] = lt > 0.f ? f2h_bits(y / lt) : (uint16_t)0;
}

struct AppendArgs {
    const uint16_t *Kn, *Vn;
    uint8_t *Kc, *Vc;
    const int32_t *kv_len;
    int64_t ldn, tok_stride, head_stride, seq_stride, items;
    int capacity, N, n_kv, D;
};

// One thread per 32 elements of one new row: a Q8_0 block (the producer's arithmetic) or 64 bytes of fp16
template <int KV>
__global__ __launch_bounds__(64) void kv_append_kernel(const AppendArgs a)
{
    const int64_t idx = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= a.items) return;
    const int nblk = a.D / 32;
    const int blk = (int)(idx % nblk);
    const int h = (int)(idx / nblk % a.n_kv);
    const int i = (int)(idx / ((int64_t)nblk * a.n_kv) % a.N);
    const int b = (int)(idx / ((int64_t)nblk * a.n_kv * a.N));
    const int pos = a.kv_len[b] - a.N + i;
    if (pos < 0 || pos >= a.capacity) return; // the caller's error: nothing outside the cache is written
    const int64_t src = ((int64_t)b * a.N + i) * a.ldn + (int64_t)h * a.D + 32 * blk;
    const int64_t dst = (int64_t)b * a.seq_stride + (int64_t)h * a.head_stride + (int64_t)pos * a.tok_stride + (KV ? 34 : 64) * blk;
    if constexpr (KV) {
        qblk::q8_block<false>(a.Kn + src, a.Kc + dst);
        qblk::q8_block<false>(a.Vn + src, a.Vc + dst);
    } else {
        uint16_t *kd = (uint16_t *)(a.Kc + dst), *vd = (uint16_t *)(a.Vc + dst);
        for (int e = 0; e < 32; ++e) kd[e] = a.Kn[src + e], vd[e] = a.Vn[src + e];
    }
}

} // namespace

AttnPlan plan_attn(int64_t B, int64_t N, int64_t n_head, int64_t n_kv_head, int64_t D, int64_t window)
{
    AttnPlan p;
    if (B <= 0 || N <= 0 || n_head <= 0 || n_kv_head <= 0 || (D != 64 && D != 128 && D != 256) || n_head % n_kv_head != 0) return p;
    const int64_t G = n_head / n_kv_head, R = N * G, BH = B * n_kv_head;
    if (R > 32 || BH > (1 << 20)) return p;
    p.ok = true;
    p.R = (int)R;
    // one workgroup per compute unit (the fp16 D = 128 ring fills its LDS), spread over the (b, h)
    const int64_t cus = num_cus(), pin = tuning().attn_w;
    int64_t W = pin > 0 ? pin : (cus / BH < 1 ? 1 : (cus / BH > kAttnMaxW ? kAttnMaxW : cus / BH));
    // a window: no more workgroups than the tiles its window + N - 1 positions can touch (one more when they straddle)
    const int64_t wtiles = window > 0 ? (window + N - 2) / kAttnTile + 2 : W;
    if (pin <= 0 && wtiles < W) W = wtiles;
    p.W = (int)W;
    p.grid = (int)(BH * W);
    // sized by a bound on BH * W that grows with B and n_kv_head: min(kAttnMaxW BH, max(BH, cus))
    const int64_t slots = pin > 0 ? BH * W : (kAttnMaxW * BH < (BH > cus ? BH : cus) ? kAttnMaxW * BH : (BH > cus ? BH : cus));
    p.workspace_bytes = (size_t)(slots * attn_slot_floats(R, D) * 4);
    return p;
}

hipError_t launch_attn_decode(int kv, const AttnCall &c, const AttnPlan &p, hipStream_t s)
{
    AttnArgs a{};
    a.Q = (const uint16_t *)c.Q, a.Kc = (const uint8_t *)c.Kc, a.Vc = (const uint8_t *)c.Vc, a.kv_len = c.kv_len;
    a.O = (uint16_t *)c.O, a.ws = (float *)c.workspace;
    a.ldq = c.ldq, a.ldo = c.ldo, a.tok_stride = c.tok_stride, a.head_stride = c.head_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.G = (int)(c.n_head / c.n_kv_head), a.n_kv = (int)c.n_kv_head, a.W = p.W;
    a.c = c.scale * 1.4426950408889634f;
    a.window = (int)c.window; // (the entry passes 0 for a window of the capacity or more: it bounds nothing)
    const bool cap = c.softcap > 0.f;
    if (cap) a.cx = softcap_consts(c.scale, c.softcap).cx, a.cc = softcap_consts(c.scale, c.softcap).cc;
    const dim3 grid((unsigned)p.grid), block(256);
    const int rt = p.R > 16 ? 2 : 1;
#define GQ_ATTN(KV, D, RT) (cap ? attn_decode_kernel<KV, D, RT, true><<<grid, block, 0, s>>>(a) : attn_decode_kernel<KV, D, RT, false><<<grid, block, 0, s>>>(a))
#define GQ_ATTN_D(KV, RT) (c.D == 256 ? GQ_ATTN(KV, 256, RT) : c.D == 128 ? GQ_ATTN(KV, 128, RT) : GQ_ATTN(KV, 64, RT))
    if (kv == 0) rt == 2 ? GQ_ATTN_D(0, 2) : GQ_ATTN_D(0, 1);
    else rt == 2 ? GQ_ATTN_D(1, 2) : GQ_ATTN_D(1, 1);
#undef GQ_ATTN_D
#undef GQ_ATTN
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 cgrid((unsigned)(c.B * c.n_kv_head * p.R)), cblock(c.D == 256 ? 128 : 64);
    if (c.D == 256) attn_combine_kernel<256><<<cgrid, cblock, 0, s>>>(a);
    else if (c.D == 128) attn_combine_kernel<128><<<cgrid, cblock, 0, s>>>(a);
    else attn_combine_kernel<64><<<cgrid, cblock, 0, s>>>(a);
    return hipGetLastError();
}

hipError_t launch_kv_append(int kv, const void *Kn, const void *Vn, int64_t ldn, void *Kc, void *Vc, int64_t tok_stride,
                            int64_t head_stride, int64_t seq_stride, const int32_t *kv_len, int64_t capacity, int64_t B,
                            int64_t N, int64_t n_kv_head, int64_t D, hipStream_t s)
{
    AppendArgs a{};
    a.Kn = (const uint16_t *)Kn, a.Vn = (const uint16_t *)Vn, a.Kc = (uint8_t *)Kc, a.Vc = (uint8_t *)Vc, a.kv_len = kv_len;
    a.ldn = ldn, a.tok_stride = tok_stride, a.head_stride = head_stride, a.seq_stride = seq_stride;
    a.items = B * N * n_kv_head * (D / 32);
    a.capacity = (int)capacity, a.N = (int)N, a.n_kv = (int)n_kv_head, a.D = (int)D;
    if (a.items == 0) return hipSuccess;
    const dim3 grid((unsigned)((a.items + 63) / 64)), block(64);
    if (kv) kv_append_kernel<1><<<grid, block, 0, s>>>(a);
    else kv_append_kernel<0><<<grid, block, 0, s>>>(a);
    return hipGetLastError();
}

} // namespace gq

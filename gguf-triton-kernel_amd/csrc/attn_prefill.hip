// attn_prefill.hip -- causal softmax attention of the N tokens last appended to each sequence over
// that sequence's fp16 or Q8_0 KV cache, for N in the hundreds or thousands (gq_attn_prefill).  The
// cache layout, the kv_len semantics, the buffer-resource bounds and the arithmetic are
// attn_decode.hip's; the work split is not.  No reference counterpart.
//
// Work split.  The R = N * G query rows of a kv head keep decode's order (row r = token r / G, head
// h G + r % G), so one pass over K and V serves all G query heads.  A workgroup of 4 waves owns ROWS =
// 64 or 128 consecutive rows of one (b, h); wave v owns rows 16 RT v .. 16 RT (v + 1) of the block
// (RT = 1 or 2 MFMA row tiles) and finishes their softmax alone: nothing is split along the keys, there
// is no workspace and no combine, O is rounded to fp16 once and stored.  The grid, B * n_kv_head *
// ceil(R / ROWS), depends on no length.  blockIdx counts the row blocks from the last one down (all
// (b, h) of the last block first): the blocks with the most keys start first and the short ones fill
// the tail.  ROWS = 128 halves the LDS reads per MFMA and is taken where it still leaves a workgroup
// for every compute unit (plan_attn_prefill); few-row shapes underfill the chip either way.
//
// Ring.  The four waves share each K/V tile: a ring of kPrefillSlots slots, each a K tile and a V tile
// of kPrefillTile keys, filled by LDS-DMA (dma16) with every wave issuing its quarter of each tile.
// Per tile i: s_waitcnt vmcnt(0) (the wave's own quarter of tile i -- the only DMAs it has in flight),
// ONE workgroup barrier (tile i has landed for everybody, and everybody has finished tile i - 1, whose
// slot tile i + 1 goes into), issue tile i + 1, compute tile i.  So K and V of tile i + 1 are both in
// flight under all of tile i's MFMAs; only a workgroup's first tile is waited for in the open.
//
// Causality is skipped, not only masked.  A workgroup walks the tiles up to its last row's limit and
// fetches no key beyond it; a wave skips the MFMAs of a 32-key step wholly beyond its own last row's
// limit (wave-uniform; it still issues its DMA quarter and meets the barrier), and the per-element
// compare runs only in steps that reach beyond the wave's FIRST row's limit.
//
// Products, per 32-key step, as in decode: keys in the A operand of v_mfma_f32_16x16x32_f16 for both
//   S^T[key 4g + i][row c] = sum_d K[key][d] Q[row][d]     A = K rows (d contiguous), B = Q (registers)
//   O^T[d 4g + i][row c]  += sum_key V[key][d] P[row][key]  A = V^T, B = P
// with k-slot 8g + j of the second product DEFINED as key (j < 4 ? 4g + j : 12 + 4g + j), which is
// what the two S^T accumulators leave in lane (g, c).  fp16 V^T comes from two transposing LDS reads
// (ds_read_b64_tr_b16: the 16 lanes of a group read keys 4g .. 4g + 3 x 16 columns as 8-byte pieces
// and each receives its column's four keys; 2 LDS reads per MFMA group instead of 8, and 76 fewer
// VGPRs at D = 128 with two row tiles), or, with the GQ_ATTN_TRV=0 tuning, from decode's element-wise
// gather -- kept as the measured alternative.  Decode's swizzle serves the transposing read unchanged:
// the 16 rows x 32 bytes a wave reads cover every bank twice, which is what 512 bytes cost anyway.
// Q8_0 keeps the byte gather.  LDS rows: decode's swizzled 16-byte pieces (fp16), raw 34-byte blocks
// in 144 / 80-byte rows (Q8_0).
//
// D = 256 (Gemma): a slot holds ONE 32-key step (PTile::TK = 32), so the fp16 ring is 2 x 2 x 16 KiB =
// 64 KiB as at D = 128 and two workgroups still fit a compute unit's LDS (Q8_0: 2 x 2 x 12 KiB); the
// barrier then comes once per 32 keys.  512-byte rows keep decode's piece ^ (row & 15) swizzle.
//
// Sliding window (gq_attn_opts.window > 0; attn_decode.hip has the rule).  A workgroup starts at the
// tile that holds its FIRST row's window start and fetches no row before it; a wave skips the steps
// that end before its own FIRST row's window start -- the earliest of its rows' starts -- (wave-uniform,
// like the causal skip), and the lower-bound compare runs only in steps that begin before its LAST
// row's start, the latest.  Soft-cap: the CAP instantiations, decode's
// formula.
#include "gguf_attn.hpp"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"
#include "gguf_mfma.hpp"

namespace gq {
namespace {

constexpr int kWaves = 4;
constexpr int kStep = 32; // keys per step of the second product
constexpr float kNegInf = -__builtin_huge_valf();
typedef short s16x4 __attribute__((ext_vector_type(4)));

struct PrefillArgs {
    const uint16_t *Q;
    const uint8_t *Kc, *Vc;
    const int32_t *kv_len;
    uint16_t *O;
    int64_t ldq, ldo, tok_stride, head_stride, seq_stride;
    int capacity, N, G, n_kv, nblk, nbh, o8;
    int window;   // 0: unbounded
    float c;      // scale * log2(e): scores are kept in the exp2 domain
    float cx, cc; // soft-cap: 2 log2(e) scale / cap and cap log2(e)
};

template <int KV, int D> struct PTile {
    static constexpr int TK = prefill_tile(D);                               // keys per ring slot
    static constexpr int RB = KV ? 34 * (D / 32) : 2 * D;                    // bytes of a cache row
    static constexpr int PPR = (RB + 15) / 16;                               // 16-byte pieces per LDS row
    static constexpr int ROWB = 16 * PPR;
    static constexpr int NIW = ((TK * PPR + 63) / 64 + kWaves - 1) / kWaves; // DMAs per wave per K (or V) tile
    static constexpr int TILEB = 1024 * kWaves * NIW;
    static constexpr int SLOT = 2 * TILEB;                                   // K tile, V tile
    static constexpr int RING = kPrefillSlots * SLOT;
};


template <int KV, int D, int RT, bool TRV, bool CAP>
__global__ __launch_bounds__(256) void attn_prefill_kernel(const PrefillArgs a)
{
    using T = PTile<KV, D>;
    constexpr int WR = 16 * RT, ROWS = kWaves * WR, NIW = T::NIW, KS = D / 32, NG = D / 16, TK = T::TK;
    __shared__ __attribute__((aligned(16))) uint8_t smem[T::RING];

    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, c = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the last row block (the most keys) first
    const int rb = a.nblk - 1 - (int)(blockIdx.x / (unsigned)a.nbh), bh = (int)(blockIdx.x % (unsigned)a.nbh);
    const int h = bh % a.n_kv, b = bh / a.n_kv;
    const int R = a.N * a.G;
    int len = a.kv_len[b];
    len = len < 0 ? 0 : (len > a.capacity ? a.capacity : len); // never outside the cache
    // keys the block's last row attends (0: none of its rows attends anything), and the waves' own limits
    const int r0 = rb * ROWS, rlast = (r0 + ROWS < R ? r0 + ROWS : R) - 1;
    int nkeys = len - a.N + rlast / a.G + 1;
    nkeys = nkeys < 0 ? 0 : nkeys;
    const int ntiles = (nkeys + TK - 1) / TK;
    const int wr0 = r0 + wave * WR, wlast = (wr0 + WR < R ? wr0 + WR : R) - 1;
    const int wmin = wr0 < R ? len - a.N + wr0 / a.G : -1, wmax = wr0 < R ? len - a.N + wlast / a.G : -1;
    // the window starts (0 without a window) of the block's first row -- nothing before it is fetched -- and
    // of the wave's first and last rows: no row of the wave attends a key before wlo0, every row all keys from wlo1
    const int wnd = a.window, pfirst = len - a.N + r0 / a.G;
    const int klo = wnd > 0 && pfirst - wnd + 1 > 0 ? pfirst - wnd + 1 : 0, tfirst = klo / TK;
    const int wlo0 = wnd > 0 && wmin - wnd + 1 > 0 ? wmin - wnd + 1 : 0, wlo1 = wnd > 0 && wmax - wnd + 1 > 0 ? wmax - wnd + 1 : 0;

    // ---- Q fragments, and the last key each of the lane's rows attends ----
    f16x8 qf[RT][KS];
    int lim[RT], lo[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = wr0 + 16 * rt + c;
        const bool live = r < R;
        const int tok = live ? r / a.G : 0, jh = live ? r - tok * a.G : 0;
        lim[rt] = live ? len - a.N + tok : -1;
        lo[rt] = wnd > 0 ? lim[rt] - wnd + 1 : 0; // (negative: no lower bound)
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

    // ---- the wave's quarter of a tile's DMA: LDS piece 64 (NIW wave + k) + lane <- (row, source piece) ----
    const uint32_t span = (uint32_t)((int64_t)(a.capacity - 1) * a.tok_stride + T::RB); // host: < 2^31
    const int64_t base = (int64_t)b * a.seq_stride + (int64_t)h * a.head_stride;
    const __amdgpu_buffer_rsrc_t krs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.Kc + base), 0, (int)span, 0x00020000);
    const __amdgpu_buffer_rsrc_t vrs = __builtin_amdgcn_make_buffer_rsrc((void *)(a.Vc + base), 0, (int)span, 0x00020000);
    int drow[NIW];
    uint32_t doff[NIW];
#pragma unroll
    for (int k = 0; k < NIW; ++k) {
        const int s = 64 * (NIW * wave + k) + lane, r = s / T::PPR, p = s - r * T::PPR;
        drow[k] = r < TK ? r : 0x40000000; // (Q8_0: the spare lanes past the tile fetch nothing)
        doff[k] = (uint32_t)(r & (TK - 1)) * (uint32_t)a.tok_stride + 16u * (uint32_t)(KV ? p : (p ^ f16_swz<D>(r)));
    }
    auto issue = [&](int t) {
        uint8_t *dst = smem + (t % kPrefillSlots) * T::SLOT + 1024 * NIW * wave;
        const uint32_t tb = (uint32_t)t * TK * (uint32_t)a.tok_stride;
        uint32_t off[NIW];
#pragma unroll
        for (int k = 0; k < NIW; ++k) { // a spare lane, a row no row of the block attends: outside the resource -- zeros, no access
            const int key = t * TK + drow[k];
            off[k] = key < nkeys && key >= klo ? tb + doff[k] : 0x80000000u;
        }
#pragma unroll
        for (int k = 0; k < NIW; ++k) dma16(krs, dst + 1024 * k, off[k], 0);
#pragma unroll
        for (int k = 0; k < NIW; ++k) dma16(vrs, dst + T::TILEB + 1024 * k, off[k], 0);
    };

    float m[RT], l[RT];
    f32x4 o[RT][NG];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        m[rt] = kNegInf, l[rt] = 0.f;
#pragma unroll
        for (int n = 0; n < NG; ++n) o[rt][n] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    // key rows (within a step) of the lane's 8 k-slots in the second product
    int vrow[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) vrow[j] = j < 4 ? 4 * g + j : 12 + 4 * g + j;

    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // Q has arrived: from here vmcnt counts DMAs only
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[rt][ks])); // (used here: no wait for Q inside the loop)
    if (ntiles > tfirst) issue(tfirst);
    for (int i = tfirst; i < ntiles; ++i) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's quarter of tile i
        __syncthreads();                                  // tile i has landed; tile i - 1's slot is drained
        if (i + 1 < ntiles) issue(i + 1);
        const uint8_t *Kt0 = smem + (i % kPrefillSlots) * T::SLOT;
#pragma unroll
        for (int st = 0; st < TK / kStep; ++st) {
            const int key0 = i * TK + st * kStep;
            if (key0 > wmax || key0 + kStep <= wlo0) continue; // wholly beyond this wave's rows, or before all their windows (wave-uniform)
            const uint8_t *Kt = Kt0 + st * kStep * T::ROWB, *Vt = Kt + T::TILEB;

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
                        float dk[4]; // block scales of the accumulator's keys 16u + 4g + e
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

            // ---- online softmax in fp32, per row (a row's four lanes g hold 8 keys each) ----
            const bool crosses = key0 + kStep - 1 > wmin; // some row of the wave ends inside this step
            const bool starts = key0 < wlo1;              // some row's window starts inside or after it
            f16x8 pf[RT];
            float p[RT][8];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                float sc[8], mx = kNegInf;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float sv = s[j >> 2][rt][j & 3];
                    sc[j] = CAP ? capped(sv * a.cx, a.cc) : sv * a.c;
                    if (crosses && key0 + vrow[j] > lim[rt]) sc[j] = kNegInf;
                    if (starts && key0 + vrow[j] < lo[rt]) sc[j] = kNegInf;
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
            if constexpr (KV == 0) {
#pragma unroll
                for (int n = 0; n < NG; ++n) {
                    f16x8 vf;
                    if constexpr (TRV) {
                        // lane c of group g sends rows 4g + c / 4 and 16 more, columns 16n + 4 (c % 4) .. + 3, and
                        // receives column 16n + c of the group's four rows: k-slots 8g .. 8g + 3, then 8g + 4 .. + 7
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
        }
        asm volatile("" ::: "memory"); // the slot's reads stay above the barrier that frees it
    }

    // ---- a row's four lanes g hold its sum in parts and 4 of every 16 columns: o / l, rounded once ----
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        float lt = l[rt];
        lt += xor_lanes(lt, 16);
        lt += xor_lanes(lt, 32);
        const float inv = lt > 0.f ? 1.0f / lt : 0.f; // (no key attended, the caller's kv_len < N: zeros)
        const int r = wr0 + 16 * rt + c;
        if (r >= R) continue;
        const int tok = r / a.G, jh = r - tok * a.G;
        uint16_t *out = a.O + ((int64_t)b * a.N + tok) * a.ldo + ((int64_t)h * a.G + jh) * D + 4 * g;
#pragma unroll
        for (int n = 0; n < NG; ++n) {
            const f32x4 v = o[rt][n] * inv;
            const uint32_t lo = (uint32_t)f2h_bits(v[0]) | ((uint32_t)f2h_bits(v[1]) << 16);
            const uint32_t hi = (uint32_t)f2h_bits(v[2]) | ((uint32_t)f2h_bits(v[3]) << 16);
            if (a.o8) *(u32x2 *)(out + 16 * n) = (u32x2){lo, hi};
            else out[16 * n] = (uint16_t)lo, out[16 * n + 1] = (uint16_t)(lo >> 16), out[16 * n + 2] = (uint16_t)hi, out[16 * n + 3] = (uint16_t)(hi >> 16);
        }
    }
}

} // namespace

PrefillPlan plan_attn_prefill(int64_t B, int64_t N, int64_t n_head, int64_t n_kv_head, int64_t D)
{
    PrefillPlan p;
    if (B <= 0 || N <= 0 || n_head <= 0 || n_kv_head <= 0 || (D != 64 && D != 128 && D != 256) || n_head % n_kv_head != 0) return p;
    if (B > INT32_MAX / n_kv_head || N > INT32_MAX / (n_head / n_kv_head)) return p;
    const int64_t R = N * (n_head / n_kv_head), BH = B * n_kv_head;
    // 128 rows where every compute unit still gets a workgroup, 64 otherwise
    const bool wide = BH * ((R + 127) / 128) >= num_cus();
    p.rows = wide ? 128 : 64;
    p.nblk = (int)((R + p.rows - 1) / p.rows);
    p.grid = BH * p.nblk;
    p.ok = p.grid <= INT32_MAX;
    return p;
}

hipError_t launch_attn_prefill(int kv, const AttnCall &c, const PrefillPlan &p, hipStream_t s)
{
    PrefillArgs a{};
    a.Q = (const uint16_t *)c.Q, a.Kc = (const uint8_t *)c.Kc, a.Vc = (const uint8_t *)c.Vc, a.kv_len = c.kv_len;
    a.O = (uint16_t *)c.O;
    a.ldq = c.ldq, a.ldo = c.ldo, a.tok_stride = c.tok_stride, a.head_stride = c.head_stride, a.seq_stride = c.seq_stride;
    a.capacity = (int)c.capacity, a.N = (int)c.N, a.G = (int)(c.n_head / c.n_kv_head), a.n_kv = (int)c.n_kv_head;
    a.nblk = p.nblk, a.nbh = (int)(c.B * c.n_kv_head);
    a.o8 = (((uintptr_t)c.O | (uintptr_t)(2 * c.ldo)) & 7) == 0; // 8-byte stores of 4 columns
    a.c = c.scale * 1.4426950408889634f;
    a.window = (int)c.window; // (the entry passes 0 for a window of the capacity or more: it bounds nothing)
    const bool cap = c.softcap > 0.f;
    if (cap) a.cx = softcap_consts(c.scale, c.softcap).cx, a.cc = softcap_consts(c.scale, c.softcap).cc;
    const dim3 grid((unsigned)p.grid), block(256);
    const bool trv = tuning().attn_trv != 0;
#define GQ_PREFILL_RT(KV, D, RT, TRV) (cap ? attn_prefill_kernel<KV, D, RT, TRV, true><<<grid, block, 0, s>>>(a) : attn_prefill_kernel<KV, D, RT, TRV, false><<<grid, block, 0, s>>>(a))
#define GQ_PREFILL(KV, D, TRV) (p.rows == 128 ? GQ_PREFILL_RT(KV, D, 2, TRV) : GQ_PREFILL_RT(KV, D, 1, TRV))
#define GQ_PREFILL_D(KV, TRV) (c.D == 256 ? GQ_PREFILL(KV, 256, TRV) : c.D == 128 ? GQ_PREFILL(KV, 128, TRV) : GQ_PREFILL(KV, 64, TRV))
    if (kv == 0) trv ? GQ_PREFILL_D(0, true) : GQ_PREFILL_D(0, false);
    else GQ_PREFILL_D(1, false);
#undef GQ_PREFILL_D
#undef GQ_PREFILL
#undef GQ_PREFILL_RT
    return hipGetLastError();
}

} // namespace gq

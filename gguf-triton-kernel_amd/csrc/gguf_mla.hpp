// gguf_mla.hpp -- what attn_mla.hip (decode) and attn_mla_prefill.hip share beside the arithmetic their
// headers describe: the geometry of a tile of kMlaTile latent cache rows in LDS, the row swizzle
// (attn_mla.hip's header has the bank argument), the addressing of a tile's LDS-DMA pieces and the LDS
// offsets of the two products' fragment reads.  Moved here from attn_mla.hip, not copied.
#pragma once
#include "gguf_internal.hpp"

namespace gq {

constexpr int kMlaWaves = 4;
constexpr int kMlaDk = kMlaRank + kMlaRope;
constexpr int kMlaRowB = 2 * kMlaDk;                              // 1152 bytes of a cache row
constexpr int kMlaPPR = kMlaRowB / 16;                            // 72 16-byte pieces per row
constexpr int kMlaNI = kMlaTile * kMlaPPR / (64 * kMlaWaves);     // 9 DMAs per lane and tile
constexpr int kMlaTileB = kMlaTile * kMlaRowB;                    // 36 KiB
constexpr int kMlaKS = kMlaDk / 32, kMlaNG = kMlaRank / 16;       // k-steps of the first product, column groups of the second
static_assert(kMlaTile == 32 && kMlaTile * kMlaPPR % (64 * kMlaWaves) == 0 && kMlaTileB % 256 == 0, "tile geometry");

// LDS piece of source piece p of tile row r (an involution: the DMA uses it the other way round)
__device__ __forceinline__ int mla_piece(int p, int r) { return p ^ ((r >> 1) & 7); }

// The k-th of a lane's kMlaNI pieces of a tile's DMA: LDS piece 256 k + tid <- (tile row, source piece).
// row: the tile row; off: its byte offset from the tile's first cache row.
__device__ __forceinline__ void mla_dma_piece(int k, int tid, int64_t tok_stride, int &row, uint32_t &off)
{
    const int s = 256 * k + tid;
    row = s / kMlaPPR;
    off = (uint32_t)row * (uint32_t)tok_stride + 16u * (uint32_t)mla_piece(s - row * kMlaPPR, row);
}

// LDS offsets within a tile of lane (g, c)'s fragment reads.  The swizzle's row term is the same for a lane's
// rows 16u + c, (c >> 1) & 7, and for its rows 16u + 4g + c / 4 of the transposing read, 2g + (c >> 3); it
// touches a piece's low 3 bits only, so pieces 8j + x of a row lie 128 j bytes apart whatever the lane: two
// bases serve the first product's 18 k-steps (k-steps 2j and 2j + 1 at mla_kbase(0 / 1) + 128 j) and four the
// second's 32 column groups (group 4q + i at mla_vbase(i) + 128 q); rows 16 more lie 16 kMlaRowB further.
__device__ __forceinline__ uint32_t mla_kbase(int e, int g, int c) { return (uint32_t)(c * kMlaRowB + 16 * mla_piece(4 * e + g, c)); }
__device__ __forceinline__ uint32_t mla_vbase(int i, int g, int c)
{
    const int row = 4 * g + (c >> 2);
    return (uint32_t)(row * kMlaRowB + 16 * mla_piece(2 * i + ((c >> 1) & 1), row) + 8 * (c & 1));
}

} // namespace gq

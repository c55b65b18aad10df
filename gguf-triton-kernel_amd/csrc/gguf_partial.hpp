// gguf_partial.hpp -- the fp16 split-K partial of the MFMA GEMM tiles: where its blocks and
// exponents lie in the workspace (PartLayout), and the order of values inside a block.
//
// A tile is 16 * WAVES * RG weight rows x 16 * NB tokens: wave w of the workgroup holds the RG
// 16-row groups wr = RG * w + rg, each as NB accumulators of v_mfma_f32_16x16x32_f16 (lane l,
// element i = D[row 16 * wr + 4 * (l >> 4) + i][token 16 * t + (l & 15)]).
//
// The workspace holds nblk = tiles x slots blocks (block tile * slots + slot; slots = the K
// splits, or a stream-K part's slot capacity), then nblk * WAVES int exponents.  A block is the
// tile's rows x tokens halves in accumulator order, as units: unit q = (wr * (NB / TPU) + u) * 64 +
// lane is lane's four rows of the TPU = 2 token tiles 2u, 2u + 1 (16 bytes; NB = 1: one tile,
// TPU = 1, 8 bytes), so every store instruction writes 1 KiB contiguous.  Wave w's values are
// scaled by 2^-e, e = exponent (block, w) = max(0, E - 14) for its largest |value| in
// [2^E, 2^(E+1)): they stay below 2^15, and e = 0 -- plain fp16 -- whenever every value does.
//
// Writers: gemm_kernel's pf16 epilogue (mmq_gemm.hip) and PartBlock (mmq_rgemm.hip: rgemm_kernel,
// the streaming kernels).  Readers, each summing a tile's slots in slot order in fp32 after the
// wave's 2^e, eight (or sixteen) loads in flight and the surplus of the last group zeroed:
// gemm_reduce_f16_kernel (8-byte items), reduce_grouped_kernel (pointer loads of whole units) and
// ilc_sum (sc1 buffer loads, inside the GEMM launch).  Same order, same arithmetic: same bits.
// Every one of them takes the block size, the exponent base and the descriptor's bytes from
// PartLayout and does the per-block arithmetic in its own integer widths (ilc_sum and PartBlock in
// 32-bit buffer offsets, the reduce kernels on pointers); exp_off(nblk, blk, wave) is for 64-bit
// callers -- in ilc_sum's 32-bit offsets it compiled to other machine code.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gq {

struct PartLayout {
    int rows, waves, bn; // the tile's weight rows, its workgroup's waves, its tokens (16 * NB)
    constexpr int halves() const { return rows * bn; }                                  // per block
    constexpr int block_bytes() const { return halves() * 2; }
    constexpr int64_t block_off(int64_t blk) const { return blk * block_bytes(); }      // bytes of blk blocks
    constexpr int64_t exp_off(int64_t nblk) const { return block_off(nblk); }           // the exponent array
    constexpr int64_t exp_off(int64_t nblk, int64_t blk, int64_t wave) const { return exp_off(nblk) + (blk * waves + wave) * 4; }
    // blocks and exponents, rounded up to align (a power of two)
    constexpr size_t bytes(int64_t nblk, size_t align = 1) const
    {
        return ((size_t)nblk * (halves() * 2 + waves * 4) + align - 1) & ~(align - 1);
    }
};

} // namespace gq

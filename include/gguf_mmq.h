/*
 * gguf_mmq.h -- C ABI of the MI355X GGUF mixed-precision matmul library (libgguf_mmq.so).
 *
 * Plain pointers and sizes only: no torch, no HIP types (streams are passed as void*,
 * i.e. a hipStream_t cast to void*; NULL = the default stream).  All device pointers are
 * HIP device memory on the current device.  Calls are asynchronous on `stream`, never
 * synchronise the host and never allocate (graph-capturable).
 *
 * Notation follows the reference: A is the packed weight matrix with M rows (output
 * features), B the fp16 activations with N rows (tokens), C = (A @ B^T)^T is fp16 (N, M).
 *
 * Reference interfaces these replace (PowerfulGhost/gguf-triton-kernel @ 2025-11-21):
 *   gq_mmq(GQ_Q8_0, ...)  <- kernels/mmq_q8_0.py:102  mmq_q8_0(A, B, M, N, K)
 *   gq_mmq(GQ_Q4_K, ...)  <- kernels/mmq_q4_k.py:240  mmq_q4_k(A, B, M, N, K)
 *   gq_mmq(GQ_Q6_K, ...)  <- kernels/mmq_q6_k.py:197  mmq_q6_k(A, B, M, N, K)
 *   gq_quantize_q8_1      <- utils/quantize/q8_1.py:18 quantize_to_q8_1 (on the device)
 *   gq_quantize_weights   <- utils/quantize/{q8_0.py:4, q4_k.py:87, q6_k.py:97} (on the device)
 *   gq_dequantize         <- utils/quantize/q4_k.py:125, q6_k.py:117, q8_0.py:52 dequantize (device)
 * Beyond the reference (no counterpart there):
 *   gq_*_ex(..., GQ_ACT_FP8_E4M3, ...)  the fp8 activation variant (BASELINE.json configs[4])
 *   gq_quantize_fp8                     its activation quantizer
 *   gq_mmq_id                           expert-indexed MMQ for mixture-of-experts blocks (mul_mat_id)
 *   gq_mmq_id_sorted                    the same at any pair count: device-sorted expert GEMM (prefill)
 *   gq_mmq_id_glu                       gate and up of every pair with SwiGLU in one launch (decode)
 *   gq_moe_combine                      the router-weighted sum over a block's slots
 *   gq_mmq_glu                          dense gate and up with SwiGLU in one launch (decode: a shared expert, a dense FFN)
 *   gq_moe_combine_shared               that sum plus a shared expert's term
 *   gq_moe_topk                         a block's router selection: S expert ids and weights from fp32 logits
 *   gq_moe_route                        the router product and that selection, for decode
 *   gq_rmsnorm                          residual add + RMSNorm of the hidden state, one launch
 *   gq_rmsnorm_prepare                  the same, written as gq_act_prepare's q8_1 activations
 */
#ifndef GGUF_MMQ_H
#define GGUF_MMQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* GQ_Q5_K (GGML type 13; the reference has none): 256 weights in 176 bytes, little endian --
 *   [0:2] d fp16 | [2:4] dmin fp16 | [4:16] 12 scale bytes (Q4_K's 6-bit sc_j / m_j, get_scale_min_k4)
 *   | [16:48] qh[32] | [48:176] qs[128];  element e, j = e / 32, l = e % 32:
 *   q = ((qs[32*(j/2) + l] >> 4*(j&1)) & 15) + 16*((qh[l] >> j) & 1),  w = d*sc_j*q - dmin*m_j.
 * q8_1 activations only: the fp8 variant (gq_*_ex with GQ_ACT_FP8_E4M3), gq_quantize_weights and
 * gq_mmq_grouped[_ex] at 5..32 tokens answer GQ_EUNSUPPORTED for it and launch nothing.
 * gq_version() did not change with it: a caller detects Q5_K by gq_block_bytes(GQ_Q5_K) == 176
 * (a library without it answers 210). */
/* GQ_Q3_K (GGML type 11, block_q3_K; the reference has none): 256 weights in 110 bytes, little
 * endian, rows of K/256 blocks without padding (blocks are 2-byte aligned) --
 *   [0:32] hmask[32] | [32:96] qs[64] | [96:108] scales[12] | [108:110] d fp16
 * element e, h = e / 128, j = (e % 128) / 32, l = e % 32, s = e / 16:
 *   q  = ((qs[32*h + l] >> 2*j) & 3) + 4*((hmask[l] >> (4*h + j)) & 1) - 4           (-4 .. 3)
 *   sc = ((s < 8 ? scales[s] & 15 : scales[s-8] >> 4) | ((scales[8 + s%4] >> 2*(s/4)) & 3) << 4) - 32
 *   w  = d*sc*q;  against q8_1 activations Q6_K's expression (a scale per 16 elements, no mins).
 * As GQ_Q5_K: q8_1 activations only, gq_quantize_weights and gq_mmq_grouped[_ex] at 5..32 tokens
 * answer GQ_EUNSUPPORTED and launch nothing; gq_mmq_id and gq_mmq_id_sorted take it under their
 * limits.  gq_version() did not change with it: detect it by gq_block_bytes(GQ_Q3_K) == 110
 * (a library without it answers 210). */
/* GQ_Q2_K (GGML type 10, block_q2_K; the reference has none): 256 weights in 84 bytes, little
 * endian, rows of K/256 blocks without padding (84 = 4*21: blocks and fields are 4-byte aligned) --
 *   [0:16] scales[16] | [16:80] qs[64] | [80:82] d fp16 | [82:84] dmin fp16
 * element e, h = e / 128, j = (e % 128) / 32, l = e % 32, s = e / 16:
 *   q  = (qs[32*h + l] >> 2*j) & 3                                                    (0 .. 3)
 *   sc = scales[s] & 15,  m = scales[s] >> 4                                          (0 .. 15)
 *   w  = d*sc*q - dmin*m   (d*sc*q and dmin*m are exact in fp32: one rounding);
 * against q8_1 activations, per 16 elements, dB*(d*sc*sum(q*qB) - dmin*m*sum(qB)).
 * As GQ_Q5_K and GQ_Q3_K: q8_1 activations only, gq_quantize_weights and gq_mmq_grouped[_ex] at
 * 5..32 tokens answer GQ_EUNSUPPORTED and launch nothing; gq_mmq_id and gq_mmq_id_sorted take it
 * under their limits.  gq_version() did not change with it: detect it by
 * gq_block_bytes(GQ_Q2_K) == 84 (a library without it answers 210). */
/* GQ_Q4_0 (GGML type 2, block_q4_0; the reference has none): 32 weights in 18 bytes, little endian,
 * rows of K/32 blocks without padding (blocks are 2-byte aligned; 256 weights are 144 bytes) --
 *   [0:2] d fp16 | [2:18] qs[16]
 * element j (0..15): q = qs[j] & 15; element 16 + j: q = qs[j] >> 4;  w = d*(q - 8), exact in fp32.
 * The block is a Q8_0 block with the same d and the int8 codes q - 8 in element order; against q8_1
 * activations it is Q8_0's expression on that image, per block d*dB*i with i = sum((q - 8)*qB) an
 * exact int32 (not llama.cpp's d*(dB*sum(q*qB) - 8*s) with the activation block's fp16 s, which
 * rounds differently).  K is any multiple of 32.
 * As GQ_Q5_K, GQ_Q3_K and GQ_Q2_K: q8_1 activations only, gq_mmq_grouped[_ex] at 5..32 tokens
 * answers GQ_EUNSUPPORTED and launches nothing; gq_mmq_id takes it at any K % 32 == 0 under its
 * limits, gq_mmq_id_sorted and gq_mmq_grouped_prepared at K % 256 == 0.  Unlike them it has a
 * device quantizer (gq_quantize_weights).  gq_version() did not change with it: detect it by
 * gq_block_bytes(GQ_Q4_0) == 18 (a library without it answers 210). */
typedef enum { GQ_Q8_0 = 0, GQ_Q4_K = 1, GQ_Q6_K = 2, GQ_Q5_K = 3, GQ_Q3_K = 4, GQ_Q2_K = 5, GQ_Q4_0 = 6 } gq_type;

/* How the activations are quantized before the matmul.
 *   GQ_ACT_Q8_1      the reference's semantics: q8_1 (int8 per 32 elements, utils/quantize/q8_1.py).
 *   GQ_ACT_FP8_E4M3  the fp8 variant: per 32-element block a power-of-two scale X = 2^e (e the
 *                    smallest integer with max|x| <= 448 * X; X = 1 for an all-zero block) and
 *                    OCP e4m3 (e4m3fn) codes of x / X, round to nearest even; the weights stay in
 *                    their GGUF precision (dequantized to fp16 in registers), products exact in
 *                    fp32.  Needs K % 256 == 0.  Inputs with |x| >= 61440 may round to 65536 and
 *                    overflow fp16. */
typedef enum { GQ_ACT_Q8_1 = 0, GQ_ACT_FP8_E4M3 = 1 } gq_act;

enum {
    GQ_OK = 0,
    GQ_EINVAL = 1,      /* bad argument: null pointer, K not a multiple of the block, ld too small ... */
    GQ_EHIP = 2,        /* a HIP launch failed (message in gq_last_error) */
    GQ_EUNSUPPORTED = 3 /* valid but not implemented (unknown type) */
};

/* Elements per block (32 / 256 / 256 / 256 / 256 / 256 / 32) and bytes per block (34 / 144 / 210 / 176 / 110 / 84 / 18). */
int gq_block_elems(gq_type t);
int gq_block_bytes(gq_type t);

/* Device workspace for this shape (bytes; the activation quantizer's output and split-K
 * partials): enough for gq_mmq and for gq_act_prepare + gq_mmq_prepared. */
size_t gq_mmq_workspace_size(gq_type t, int64_t M, int64_t N, int64_t K);
size_t gq_mmq_workspace_size_ex(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K);
/* The exact need of one gq_mmq_ex call (<= the above): 0 when the call is a one-launch decode
 * (its quantizer works in LDS), and then workspace may be NULL. */
size_t gq_mmq_call_workspace_size(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K);

/*
 * C[n * ldc + m] = sum_k W[m][k] * x~[n][k]  for m < M, n < N (fp16 out, fp32 accumulate)
 *   A : packed `t` weights, M rows of K/QK blocks, row m at byte m*(K/QK)*block_bytes
 *   B : fp16 activations, row n at element n*ldb (ldb >= K)
 *   x~: B quantized exactly as utils/quantize/q8_1.py does (int8 per 32 elements), the
 *       input the reference's parity oracle (kernels/cpu_impls) consumes.
 * K must be a multiple of gq_block_elems(t) (the reference asserts the same).
 * workspace: >= gq_mmq_workspace_size(t, M, N, K) bytes of device memory
 *            (exactly: gq_mmq_call_workspace_size(t, GQ_ACT_Q8_1, M, N, K); NULL when that is 0).
 * Returns GQ_OK or an error code (gq_last_error() has the text; nothing was launched).
 *
 * Pointers and strides (gq_mmq[_ex], gq_act_prepare[_ex], gq_mmq_prepared[_ex], gq_dequantize,
 * gq_quantize_q8_1, gq_quantize_fp8, gq_rmsnorm, gq_rmsnorm_prepare; tests/test_gpu_strides.py holds
 * every dense route to this, tests/test_gpu_rmsnorm.py the two norm entries):
 *   - B, C, W and X (the norm entries' X, R, H and Y) need fp16's 2-byte alignment and nothing more,
 *     and any row stride >= the row length (ldb >= K, ldc >= M, ldw >= K, ldx >= K, and ldr, ldh,
 *     ldy >= K; shorter: GQ_EINVAL).  Only the row's own K
 *     (M) elements are read (written): the ld - K pad columns, rows >= N and whatever lies in front
 *     of the base are never read into a result, and the ld - M pad columns of C are never written.
 *     A needs no alignment beyond its blocks' (a 16-byte load may read up to 15 bytes past its end).
 *   - The result does not depend on ldc or on where C starts: every ldc and base give the bits of
 *     ldc = M on an aligned base.  One exception, the K-chunked streaming MMQ, stores 8 bytes at a
 *     time through a buffer resource and takes a call only with ldc % 4 == 0 and C on an 8-byte
 *     boundary; any other C goes to the route the same call has under GQ_KSTREAM=0 (that call's
 *     bits, within the GEMM tolerance of the stream's; a grouped launch refuses the item,
 *     GQ_EUNSUPPORTED).  gq_debug_route sees the shape alone and reports the aligned call's kernel.
 *   - 16-byte rows of B (B on a 16-byte boundary and ldb % 8 == 0) select the kernels that
 *     quantize B inside their one launch (the K-chunked stream, the resident GEMM).  Any other B
 *     is quantized by act_quant first and the call is gq_mmq_prepared's: the bits of
 *     gq_act_prepare + gq_mmq_prepared on a contiguous copy.  The one-launch decode, the GEMV, the
 *     LDS-DMA GEMM and everything that reads act_quant's output take any B, with the same bits.
 *   - The workspace need does not depend on strides or alignment: exactly
 *     gq_mmq_call_workspace_size (gq_mmq_workspace_size_ex for the split form) bytes suffice for
 *     every case above, and nothing behind them is written.
 *   - Not tested: a C that is not 8-byte aligned on the dequantize + hipBLASLt route (from
 *     GQ_BLAS_MIN_TOKENS tokens); hipBLASLt is given ldc = M, M + 24 and M + 3 on aligned bases.
 */
int gq_mmq(gq_type t, const void *A, const void *B, void *C, int64_t M, int64_t N, int64_t K, int64_t ldb,
           int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);
/* gq_mmq with the activation format chosen (gq_mmq == gq_mmq_ex(t, GQ_ACT_Q8_1, ...)). */
int gq_mmq_ex(gq_type t, gq_act act, const void *A, const void *B, void *C, int64_t M, int64_t N, int64_t K,
              int64_t ldb, int64_t ldc, void *workspace, size_t workspace_bytes, void *stream);

/*
 * Split form of gq_mmq.  gq_act_prepare quantizes B into the front of `workspace` (that
 * part depends only on N and K); gq_mmq_prepared then runs the matmul for any weight
 * type and M with that K, using the rest of the workspace (which must be at least
 * gq_mmq_workspace_size(t, M, N, K) bytes in total) for split-K partial sums.  One prepare
 * can serve several weight matrices that share an input (Q/K/V, gate/up).
 * Same result as gq_mmq within the stated tolerances, not always the same kernels: for
 * N <= 4 (fp8: N <= 2) gq_act_prepare also keeps an fp16 copy of B in the workspace and
 * gq_mmq_prepared runs gq_mmq's one-launch fused decode on it -- the same kernel and bits as
 * gq_mmq (round 5; the split form ran the decode-shaped GEMV on the SOA q8_1 form before, and
 * still does where the fused decode does not fit, e.g. 4 tokens at K = 11008); at N = 5..32 (K <= 4096,
 * M % 16 == 0) the split form runs the K-chunked streaming MMQ, and gq_mmq does too at N <= 16 on
 * M >= 8192 rows, else the resident GEMM (the same x~ and products, summed over K in another fp32
 * order: within 4e-3, not bit for bit; GQ_KSTREAM=1 puts both on the stream, GQ_KSTREAM=0 both
 * off it, and then the bits match);
 * for Q8_0 with the int8 GEMM form enabled (GQ_GEMM_I8=1) gq_act_prepare writes both activation
 * forms.
 */
int gq_act_prepare(const void *B, int64_t N, int64_t K, int64_t ldb, void *workspace, size_t workspace_bytes,
                   void *stream);
int gq_mmq_prepared(gq_type t, const void *A, void *workspace, size_t workspace_bytes, void *C, int64_t M, int64_t N,
                    int64_t K, int64_t ldc, void *stream);
/* The split form with the activation format chosen (both calls must name the same one). */
int gq_act_prepare_ex(gq_act act, const void *B, int64_t N, int64_t K, int64_t ldb, void *workspace,
                      size_t workspace_bytes, void *stream);
int gq_mmq_prepared_ex(gq_type t, gq_act act, const void *A, void *workspace, size_t workspace_bytes, void *C,
                       int64_t M, int64_t N, int64_t K, int64_t ldc, void *stream);

/*
 * Several gq_act_prepare_ex calls in as few launches as possible, e.g. the four inputs of one
 * transformer block's projections (no reference counterpart: the reference quantizes inside
 * every matmul).  Item i prepares B_i (N_i x K_i fp16, row stride ldb_i) into its own
 * workspace exactly as gq_act_prepare_ex(act, B_i, ...) would -- the same bytes, the same
 * errors.  Items whose prepared form is the fp16 x~ of the GEMM paths (GQ_ACT_Q8_1 at N >= 5;
 * GQ_ACT_FP8_E4M3's widened codes at every N) share one launch per 8 items; the others are
 * prepared one by one.  Every item is checked
 * before anything is launched: a bad item (GQ_EINVAL / GQ_EUNSUPPORTED) launches nothing.
 * No host sync.
 */
typedef struct gq_prep_item {
    const void *B;
    int64_t N, K, ldb;
    void *workspace;
    size_t workspace_bytes;
} gq_prep_item;
int gq_act_prepare_grouped(gq_act act, const gq_prep_item *items, int n, void *stream);

/*
 * Dequantize packed `t` weights to fp16: W[m * ldw + k] = w (the reference's block formulas,
 * utils/quantize/{q8_0,q4_k,q6_k}.py dequantize, evaluated in fp32, rounded once to fp16).
 * GQ_Q5_K: (d*sc_j)*q - (dmin*m_j), the formula above, in that order.  GQ_Q3_K: (d*sc)*q.
 * GQ_Q2_K: (d*sc)*q - (dmin*m), one rounding.  GQ_Q4_0: d*(q - 8), exact in fp32.
 * M rows of K (a multiple of the block) elements.  gq_mmq uses the same kernel for its
 * library-GEMM path (N >= a few hundred tokens: fp16 W + hipBLASLt).
 */
int gq_dequantize(gq_type t, const void *A, void *W, int64_t M, int64_t K, int64_t ldw, void *stream);

/*
 * q8_1 quantization of fp16 rows on the device, byte-identical to utils/quantize/q8_1.py:
 * rows x K fp16 (row stride ldx elements) -> rows * K/32 blocks of 36 bytes, row-major.
 */
int gq_quantize_q8_1(const void *X, void *Y, int64_t rows, int64_t K, int64_t ldx, void *stream);

/*
 * The fp8 variant's activation quantizer (GQ_ACT_FP8_E4M3 above) on the device: rows x K fp16
 * (row stride ldx) -> codes [rows][K] e4m3fn bytes, each 4-element group stored in the order
 * (0,2,1,3), and scales [K/32][(rows + 3) & ~3] float X = 2^e (block-major).
 */
int gq_quantize_fp8(const void *X, void *codes, void *scales, int64_t rows, int64_t K, int64_t ldx, void *stream);

/*
 * GGUF weight quantization on the device (the reference quantizes on the host only), byte-
 * identical to the reference's producers and to include/gguf_quant.h's gq_quantize_*:
 *   GQ_Q8_0: X = n fp16 values (n % 32 == 0)  -> Y = n/32 blocks of 34 bytes (quantize_to_q8_0)
 *   GQ_Q4_K: X = n fp32 values (n % 256 == 0) -> Y = n/256 blocks of 144 bytes (quantize_to_q4_k)
 *   GQ_Q6_K: X = n fp32 values (n % 256 == 0) -> Y = n/256 blocks of 210 bytes (quantize_to_q6_k)
 *   GQ_Q4_0: X = n fp32 values (n % 32 == 0)  -> Y = n/32 blocks of 18 bytes (gq_quantize_q4_0; no reference)
 * GQ_Q5_K, GQ_Q3_K, GQ_Q2_K: GQ_EUNSUPPORTED (host only: include/gguf_quant.h gq_quantize_q5_k / _q3_k / _q2_k).
 * X is read as flat blocks (a row-major (M, K) matrix gives the packed A of gq_mmq).  One thread
 * per block runs the host producer's exact code; no host sync.
 */
int gq_quantize_weights(gq_type t, const void *X, void *Y, int64_t n, void *stream);

/*
 * Row-sharded MMQ over the GPUs of one node (SURVEY.md 8(b) "gq_mmq_sharded", 8(e)).  The
 * reference is single-GPU and has no counterpart; this is the C form of dist/row_shard.py.
 *
 * gq_shard_rows: rank `rank` of `world` owns weight rows [*row0, *row0 + *rows) of M, padded
 * shard size *R = ceil(M / world) rounded up to 64 (the last shards may be short or empty).
 * Its packed bytes are A + row0 * (K / gq_block_elems(t)) * gq_block_bytes(t): no repacking.
 */
int gq_shard_rows(int64_t M, int world, int rank, int64_t *row0, int64_t *rows, int64_t *R);

/*
 * (world, N, R) fp16 slabs, as an all-gather leaves them -> C (N rows of ldc), columns [0, M):
 * C[n][m] = gathered[m / R][n][m % R].  One device copy kernel on `stream`.
 */
int gq_assemble_shards(const void *gathered, void *C, int world, int64_t N, int64_t R, int64_t M, int64_t ldc,
                       void *stream);

/*
 * One rank's row-sharded MMQ: the local gq_mmq of this rank's rows (A_shard, from
 * gq_shard_rows) into an (N, R) slab, an RCCL all-gather of the slabs over `nccl_comm` (an
 * ncclComm_t of this rank, world ranks; RCCL is resolved at run time from the process, so the
 * caller's own RCCL is the one used), and gq_assemble_shards into C (N, ldc) -- every rank ends
 * with the whole output.  All on `stream`, no host sync (graph-capturable as RCCL allows).
 * world == 1 needs no communicator (NULL: no collective; a 1-rank communicator is used as given).  Workspace: at least
 * gq_mmq_sharded_workspace_size(t, M, N, K, world) bytes.
 */
size_t gq_mmq_sharded_workspace_size(gq_type t, int64_t M, int64_t N, int64_t K, int world);
int gq_mmq_sharded(gq_type t, const void *A_shard, const void *B, void *C, int64_t M, int64_t N, int64_t K,
                   int64_t ldb, int64_t ldc, int world, int rank, void *nccl_comm, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * Grouped MMQ: several MMQs of the same token count N (1..32) in one launch, e.g. the
 * projections of one transformer block at decode / small-batch time.  The reference has no
 * counterpart (its kernels/mmq_*.py take one matrix per call); this is the launch the layer
 * dispatcher (kernels/layer_mix.py) makes.  Item i: weights A (M x K of `type`),
 * fp16 activations B (N x K, row stride ldb, q8_1-quantized in the kernel as gq_mmq does), fp16
 * output C (N x M, row stride ldc); items may share B.  N = 1..4: the streaming decode kernel,
 * every item's output bit-identical to its own gq_mmq call; N = 5..32: the K-chunked streaming
 * MMQ (every item bit-identical to its own gq_mmq_ex on that kernel, GQ_KSTREAM=1), which needs
 * K % 256 == 0, K <= 4096, M % 16 == 0, B 16-byte aligned and ldb % 8 == 0, C 8-byte aligned and ldc % 4 == 0.  The chip's workgroups are split over the items by weight bytes.  No workspace, no host
 * sync.  GQ_EUNSUPPORTED (nothing launched) when N > 32, or an item is not a shape of that
 * launch (decode: activations that do not fit LDS, >= 2 GiB of weights, more than 16 parts =
 * item x token group; 5..32: the conditions above, more than 16 items): call gq_mmq per item then.
 */
typedef struct gq_group_item {
    gq_type type;
    const void *A;
    const void *B;
    int64_t ldb;
    void *C;
    int64_t ldc;
    int64_t M, K;
} gq_group_item;
int gq_mmq_grouped(const gq_group_item *items, int n, int64_t N, void *stream);
/* The same with an activation format: GQ_ACT_Q8_1 is gq_mmq_grouped; GQ_ACT_FP8_E4M3 (the fp8
 * variant: its decode form at N <= 2, the K-chunked stream at 3..32) gives every item
 * gq_mmq_ex(..., GQ_ACT_FP8_E4M3, ...)'s bits on that kernel. */
int gq_mmq_grouped_ex(gq_act act, const gq_group_item *items, int n, int64_t N, void *stream);

/*
 * Expert-indexed MMQ (llama.cpp's mul_mat_id) for mixture-of-experts blocks at decode: N tokens
 * each multiply S router-chosen experts out of E, the choices read from DEVICE memory by the
 * kernel -- no host copy of the ids, so the call keeps this header's promise (asynchronous, no
 * host sync, no allocation, graph-capturable: a replay follows whatever `ids` holds then).
 *   A        : E packed M x K matrices of `t` back to back, expert e at byte
 *              e*M*(K/QK)*block_bytes -- a GGUF 3-D tensor blk.L.ffn_*_exps.weight (dims (K, M, E))
 *              as stored, no repacking.
 *   ids      : N*S int32 in device memory; pair p = n*S + s multiplies expert ids[p].
 *   B        : fp16 activations; pair (n, s) reads the K elements at n*ldb + s*ldb_slot (ldb >= K).
 *              ldb_slot = 0: the S slots share token n's row (gate / up); ldb_slot >= K: one row
 *              per slot (down).  No alignment beyond fp16's, as gq_mmq's one-launch decode.
 *   C        : fp16; pair p's M outputs start at element p*ldc (ldc >= M).
 * Pair p's outputs are bit-identical to gq_mmq(t, A_e, row, C_p, M, 1, K, ...) on that expert
 * and row under the default tuning.  An id outside [0, E) reads no weights and gives M zeros.
 * One launch, every pair on an equal share of the chip; q8_1 activations only (no fp8 form).
 * M == 0, N == 0 or S == 0: a no-op.  GQ_EINVAL: null pointer, ldb < K, ldc < M, an ldb_slot
 * that is neither 0 nor >= K.  GQ_EUNSUPPORTED (nothing launched): more than 64 pairs (8 tokens x
 * top-8: every pair streams its expert's weights itself; beyond that, pairs that share an expert
 * should share one weight stream -- a sorted GEMM this entry is not), a K whose one-token
 * activations do not fit the decode's LDS image, or one expert of >= 2 GiB (the whole tensor may
 * be larger).  The caller then calls gq_mmq_id_sorted (below; kernels/_lib.py mmq_id does), or,
 * where that refuses too, groups the pairs by expert on the host and calls gq_mmq per expert.
 * Like gq_mmq on a row slice, the weight stream reads whole 16-byte pieces from each expert's first
 * byte: an expert that does not start 16-byte aligned may have up to 15 bytes read (never used)
 * past its end, so the last expert should not end flush with the end of mapped device memory
 * (device allocators' granularity guarantees it).
 * gq_version() did not change with it: a caller detects the entry by its symbol (dlsym).
 */
int gq_mmq_id(gq_type t, const void *A, const int32_t *ids, const void *B, void *C, int64_t E, int64_t M, int64_t N,
              int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc, void *stream);

/*
 * Sorted expert GEMM: gq_mmq_id's job at ANY pair count (prefill, batched decode) -- the same
 * arguments, the same promise (asynchronous, no host sync, no allocation, graph-capturable: a
 * replay follows whatever `ids` holds then), plus a workspace.  Three launches whose grids depend
 * on the sizes only, never on the ids:
 *   1. one workgroup sorts the N*S pairs by expert on the device (a stable counting sort: a
 *      permutation of the pair indices, ascending inside an expert's group, ids outside [0, E)
 *      last) and writes a table of (expert, first sorted row, rows) token tiles;
 *   2. the activation quantizer gathers through the permutation: sorted row r is the fp16 x~ of
 *      pair perm[r]'s row at n*ldb + s*ldb_slot -- the bytes gq_act_prepare writes for that row
 *      (no alignment beyond fp16's) -- and zeroes the M outputs of every out-of-range pair;
 *   3. the streaming GEMM (gq_mmq_prepared's 256-row MFMA kernel body, the whole K in one split)
 *      runs once per table entry and row tile -- pairs that share an expert share its weight
 *      stream -- and scatters sorted row r to C + perm[r]*ldc.  Its grid is sized for the worst
 *      case, ceil(M/256) x (min(E, N*S) + N*S / tile) workgroups; those past the table's end exit.
 * Pair p's outputs are bit-identical to its row of gq_mmq_prepared on that expert and the
 * gathered rows with the streaming GEMM pinned to one split (GQ_SGEMM=1, GQ_SGEMM_SPLITS=1), and
 * do not depend on the other pairs' ids.  q8_1 activations, all four weight types.
 * M == 0, N == 0 or S == 0: a no-op.  An id outside [0, E) reads no weights and gives M zeros.
 * GQ_EINVAL: gq_mmq_id's list, and a NULL workspace or one smaller than
 * gq_mmq_id_sorted_workspace_size(t, E, M, N, S, K) (>= N*S*K*2 bytes: the gathered x~, then the
 * permutation and the table; 0 for a shape the entry refuses or an empty one).
 * GQ_EUNSUPPORTED (nothing launched): K % 256 != 0 (the streaming GEMM works in super-blocks:
 * Q8_0 too), E > 1024, N*S > 65536, N*S*K*2 >= 4 GiB, or one expert of >= 2 GiB.
 * As gq_mmq_id, the weight stream reads whole 16-byte pieces from each expert's first byte (up to
 * 15 bytes, never used, past an expert that does not end 16-byte aligned).
 * gq_version() did not change with it: a caller detects the entry by its symbol (dlsym).
 */
size_t gq_mmq_id_sorted_workspace_size(gq_type t, int64_t E, int64_t M, int64_t N, int64_t S, int64_t K);
int gq_mmq_id_sorted(gq_type t, const void *A, const int32_t *ids, const void *B, void *C, int64_t E, int64_t M, int64_t N,
                     int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc, void *workspace,
                     size_t workspace_bytes, void *stream);

/*
 * Fused gate / up of a mixture-of-experts FFN block at decode: both expert-indexed products of
 * every (token, slot) pair and their SwiGLU in ONE launch (llama.cpp's mul_mat_id + GLU).  The
 * token's row is quantized once per workgroup and serves both weight streams.
 *   A_gate, A_up : two expert tensors of the same type `t`, E, M and K, each laid out as
 *                  gq_mmq_id's A.
 *   ids, B, ldb, ldb_slot : as gq_mmq_id.
 *   H            : fp16; pair p's M values start at element p*ldh (ldh >= M).
 * Defined result, for pair p and row m: with g and u the fp16 values, bit for bit, that gq_mmq_id
 * writes for that pair and row from A_gate and from A_up,
 *   H = fp16_rne( (float)g / (1 + expf(-(float)g)) * (float)u )
 * evaluated in fp32 and rounded once.  (g and u are rounded to fp16 first on purpose: the fused
 * entry is a function of bits the library already produces.)  An id outside [0, E) reads no
 * weights and writes M zeros.
 * Limits, checks, return codes and their order are gq_mmq_id's (at most 64 pairs, a K that fits
 * the one-token decode, q8_1 activations only, one expert < 2 GiB; a null A_up is a null pointer).
 * GQ_EUNSUPPORTED launches nothing and leaves H untouched: the caller then makes the same result
 * from two gq_mmq_id (or gq_mmq_id_sorted) calls (kernels/_lib.py mmq_id_glu does).
 * Asynchronous, no host sync, no allocation, graph-capturable: a replay follows `ids`.
 * gq_version() did not change with it: a caller detects the entry by its symbol (dlsym).
 */
int gq_mmq_id_glu(gq_type t, const void *A_gate, const void *A_up, const int32_t *ids, const void *B, void *H, int64_t E,
                  int64_t M, int64_t N, int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldh, void *stream);

/*
 * The router-weighted sum over slots that ends a mixture-of-experts block, one launch:
 *   D : fp16, pair p = n*S + s's M values at element p*ldd (ldd >= M) -- gq_mmq_id's output of
 *       the down projection.
 *   W : N*S router weights, fp16 (w_is_f32 == 0) or fp32 (w_is_f32 != 0), pair p's at W[p].
 *   Y : fp16 (N, M), token n's row at element n*ldy (ldy >= M).
 * Y[n][m] = fp16_rne(acc), acc = 0.f and, for s = 0..S-1 in that order, acc = acc + w*d with the
 * product and the sum each rounded to fp32 (no fused multiply-add); with fp16 weights the product
 * is exact.  Deterministic: every output is summed by one thread in slot order, no atomics.
 * Any N, S <= 64, M < 2^31.  N == 0, S == 0 or M == 0: a no-op.  GQ_EINVAL: a negative size, a
 * null pointer, ldd < M, ldy < M.  GQ_EUNSUPPORTED (nothing launched): S > 64 or M >= 2^31.
 * Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol.
 */
int gq_moe_combine(const void *D, const void *W, int w_is_f32, void *Y, int64_t N, int64_t S, int64_t M, int64_t ldd,
                   int64_t ldy, void *stream);

/*
 * Dense gate / up with SwiGLU at decode, ONE launch: the FFN of a dense model and the shared expert
 * of a mixture-of-experts block.  The tokens are quantized once per workgroup and serve both
 * weight streams.
 *   A_gate, A_up : two packed M x K matrices of the same type `t`, each as gq_mmq's A.
 *   B            : fp16 (N, K), row stride ldb >= K, no alignment beyond fp16's.
 *   H            : fp16 (N, M), row stride ldh >= M.
 * Defined result (gq_mmq_id_glu's definition): with g and u the fp16 values, bit for bit, that
 * gq_mmq(t, A_gate | A_up, B, ..., M, N, K, ...) writes at this N under the default tuning,
 *   H = fp16_rne( (float)g / (1 + expf(-(float)g)) * (float)u )
 * evaluated in fp32 and rounded once.
 * It takes 1 <= N <= 4 tokens (q8_1 activations) at the shapes where gq_mmq's own route for
 * (t, M, N, K) is the one-launch decode, each matrix under 2 GiB.  GQ_EUNSUPPORTED launches
 * nothing and leaves H untouched: N > 4; a K whose tokens do not fit the decode's LDS image (the
 * GEMV shapes, e.g. 4 tokens at K >= 8960 for Q3_K); a matrix >= 2 GiB; a shape whose stash of g
 * values would cost the launch a workgroup per CU; a shape whose kernel is not built because it
 * would spill registers ("Dense GLU decode and shared experts").  The caller then
 * makes the same result from two gq_mmq calls (kernels/_lib.py mmq_glu does).
 * GQ_EINVAL: a null pointer, a negative size, ldb < K, ldh < M, K not a multiple of the block.
 * M == 0 or N == 0: a no-op.  No workspace.  Asynchronous, no host sync, no allocation,
 * graph-capturable.
 * gq_version() did not change with it: a caller detects the entry by its symbol (dlsym).
 */
int gq_mmq_glu(gq_type t, const void *A_gate, const void *A_up, const void *B, void *H, int64_t M, int64_t N, int64_t K,
               int64_t ldb, int64_t ldh, void *stream);

/*
 * gq_moe_combine with a shared expert's term, one launch:
 *   D, W, w_is_f32, Y, ldd, ldy : exactly gq_moe_combine's.
 *   Dsh  : fp16 (N, M), token n's M values at element n*ldsh (ldsh >= M) -- the shared expert's
 *          down output.
 *   gate : NULL, or N fp32 values in device memory (Qwen-MoE's per-token sigmoid gate).
 * Y[n][m] = fp16_rne(acc): acc = 0.f; for s = 0..S-1 in that order acc = acc + w*d, the product and
 * the sum each rounded to fp32 (gq_moe_combine's order); then acc = acc + dsh, or with a gate
 * acc = acc + gate[n]*dsh, again a rounded product and a rounded sum (no fused multiply-add).
 * Deterministic: one thread per output, no atomics.
 * Any N, 1 <= S <= 64, M < 2^31.  N == 0 or M == 0: a no-op.  GQ_EINVAL: S == 0 (with a shared term
 * an empty sum is not a no-op), a negative size, a null D, W, Dsh or Y, ldd, ldsh or ldy < M.
 * GQ_EUNSUPPORTED (nothing launched): S > 64 or M >= 2^31.
 * Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol.
 */
int gq_moe_combine_shared(const void *D, const void *W, int w_is_f32, const void *Dsh, int64_t ldsh, const float *gate,
                          void *Y, int64_t N, int64_t S, int64_t M, int64_t ldd, int64_t ldy, void *stream);

/*
 * The router's selection, one launch at any N: from each token's E fp32 logits to its S expert ids
 * and their weights, the two arrays gq_mmq_id[_glu|_sorted] and gq_moe_combine read.
 *   logits : fp32, token n's E values at element n*ldl (ldl >= E).
 *   bias   : NULL, or E fp32 selection biases (func 1 only).
 *   ids    : int32 (N, S), token n's at ids[n*S].      W : (N, S), fp32 (w_is_f32 != 0) or fp16.
 * Key of expert e, with L its logit:   func 0 (softmax): L.   func 1 (sigmoid): L without a bias
 * (sigmoid is monotone; selecting on L makes no ties that rounding would), else
 * s_e + bias[e] in fp32 with s_e = 1 / (1 + expf(-L)).
 * Selection: the S experts of largest key in descending key order, the lower index first among
 * equal keys (-0 equals +0), a NaN key below every number.  Whatever the logits hold, the ids are S
 * distinct values in [0, E).
 * Value v_e: func 0, softmax(L)_e over all E experts in fp32 with the row maximum subtracted;
 * func 1, s_e (the bias selects, it never weighs).  Weight of slot s: v_{id_s}, divided by the sum
 * of the S selected values when norm != 0, times scale, rounded once to W's type.  (With func 0
 * and norm the softmax denominator cancels and is not formed.)  Weights are meant for finite
 * logits; a row with NaN or infinite entries still gets valid ids.
 * N == 0: a no-op.  GQ_EINVAL: a negative size, a null logits / ids / W, ldl < E, func not 0 or 1,
 * a bias with func 0.  GQ_EUNSUPPORTED (nothing launched): outside 1 <= S <= E, E > 1024
 * (gq_mmq_id_sorted's limit) or S > 64 (gq_moe_combine's).
 * Deterministic (one wave per token, no atomics): a token's ids and weights depend on its own row
 * alone.  Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol.
 */
int gq_moe_topk(const float *logits, int64_t ldl, const float *bias, int func, int norm, float scale, int32_t *ids, void *W,
                int w_is_f32, int64_t N, int64_t E, int64_t S, void *stream);

/*
 * The router of a mixture-of-experts block at decode, two launches: the product with the router
 * matrix, then gq_moe_topk's selection.
 *   Wr     : the (E, H) router matrix, contiguous, fp32 (wr_is_f16 == 0; GGUF's
 *            blk.L.ffn_gate_inp.weight as stored) or fp16.
 *   X      : fp16 (N, H), token n's row at element n*ldx (ldx >= H).
 *   logits : fp32, required; the call writes L[n][e] = sum_k X[n][k] * Wr[e][k], accumulated in fp32,
 *            at element n*ldl + e.  It is the router's one piece of workspace and the caller's to keep.
 *   bias, func, norm, scale, ids, W, w_is_f32 : gq_moe_topk's, applied to exactly the stored logits.
 * The summation order of an (n, e) is fixed whatever N is: a token's logits, ids and weights are
 * the bits of its own one-token call.
 * Checks, limits and their order are gq_moe_topk's (Wr and X with the pointers, ldx < H with ldl,
 * H < 0 with the sizes), and then N <= 64 and H % 32 == 0, else GQ_EUNSUPPORTED with nothing
 * launched and nothing written: multiply outside and call gq_moe_topk (kernels/_lib.py moe_route
 * does).  Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol.
 */
int gq_moe_route(const void *Wr, int wr_is_f16, const void *X, int64_t ldx, float *logits, int64_t ldl, const float *bias,
                 int func, int norm, float scale, int32_t *ids, void *W, int w_is_f32, int64_t N, int64_t E, int64_t H,
                 int64_t S, void *stream);

/*
 * Residual add + RMSNorm of the hidden state, one launch, one workgroup per token:
 *   X : fp16 (N, K), row n at element n*ldx.       R : NULL, or the residual, fp16 (N, K), rows ldr apart.
 *   H : NULL, or fp16 (N, K), rows ldh apart: the new residual stream h.
 *   w : K fp32 values (GGUF stores *_norm.weight as F32), 4-byte aligned.
 *   Y : fp16 (N, K), rows ldy apart: the normed activations (required).
 *   h[k]  = R ? fp16_rne(float(x[k]) + float(r[k])) : x[k]
 *   ss    = sum_k float(h[k])^2 in fp32 (every square is exact; the additions in an order that is a
 *           function of K alone: 256 lanes each sum their own elements in k order, then a tree)
 *   scale = 1 / sqrtf(ss / K + eps), IEEE fp32 division and square root
 *   y[k]  = fp16_rne((float(h[k]) * scale) * w[k]), two rounded fp32 products
 * A token's h and y are the bits of its own one-token call, at every N, stride and base.
 * H may be X or R themselves (the same base and the same stride: the in-place update of the
 * residual stream).  Any other overlap of H with X or R, and Y (or w) overlapping X, R or H, is
 * GQ_EINVAL: the byte ranges are compared on the host.  Only a row's K elements are read or written.
 * K % 32 == 0, every ld >= K, eps finite and >= 0 (GQ_EINVAL otherwise, as a null X, w or Y or a
 * negative size); N == 0 or K == 0: a no-op.  N >= 2^31: GQ_EUNSUPPORTED.  Every check precedes the
 * launch.  Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol;
 * gq_version() did not change with it.
 */
int gq_rmsnorm(const void *X, const void *R, void *H, const float *w, float eps, void *Y, int64_t N, int64_t K, int64_t ldx,
               int64_t ldr, int64_t ldh, int64_t ldy, void *stream);

/*
 * gq_rmsnorm whose y goes straight into a workspace as gq_act_prepare(y, N, K, ...) would leave it
 * (GQ_ACT_Q8_1): byte for byte that call's activation part -- the decode token counts' SOA codes,
 * d and s with, where gq_act_prepare keeps one, the fp16 copy (y itself); from 5 tokens the fp16 x~
 * -- so that any number of gq_mmq_prepared calls with this (N, K) follow.  One launch: y makes no
 * round trip through memory and is quantized where it is made.
 *   Y : may be NULL (y is then not stored); otherwise gq_rmsnorm's Y, the same bits.
 *   workspace : >= gq_mmq_workspace_size(t, M, N, K) bytes for the products that follow; this call
 *               needs and writes the activation part only.  It must not overlap X, R, H, Y or w.
 * Checks: gq_rmsnorm's, then the workspace (null or short: GQ_EINVAL), then the overlaps.
 * Where gq_act_prepare also writes the int8 GEMM form (the GQ_GEMM_I8=1 tuning, from 5 tokens at
 * K % 256 == 0) this entry is gq_rmsnorm into Y followed by gq_act_prepare's launches on Y -- the
 * same bytes -- and with Y == NULL it answers GQ_EUNSUPPORTED and launches nothing: call the two
 * entries.  The fp8 activation variant is not part of this entry (gq_rmsnorm + gq_act_prepare_ex).
 * Asynchronous, no host sync, no allocation, graph-capturable.  Detected by its symbol.
 */
int gq_rmsnorm_prepare(const void *X, const void *R, void *H, const float *w, float eps, void *Y, int64_t N, int64_t K,
                       int64_t ldx, int64_t ldr, int64_t ldh, int64_t ldy, void *workspace, size_t workspace_bytes,
                       void *stream);

/*
 * Grouped GEMM: several gq_mmq_prepared_ex calls with the same token count N (5 <= N) in ONE
 * launch of the streaming 256-row MFMA GEMM (+ one launch summing the split-K partials), e.g.
 * the seven projections of a transformer block at prefill (BASELINE.json configs[4]; no
 * reference counterpart).  Item i: weights A (M x K of `type`, K % 256 == 0), ws = the
 * workspace its input was prepared into by gq_act_prepare[_ex|_grouped](act, ..., N, K, ...)
 * (items may share one), output C (N x M, row stride ldc).  The chip's workgroups are spread
 * over the items' row tiles x super-blocks (each item split along K so that the whole launch is
 * one round of the chip); with the split factor pinned (GQ_SGEMM_SPLITS) every item's output is
 * bit-identical to its own gq_mmq_prepared_ex call on that kernel (GQ_SGEMM=1).  At N = 5..32
 * the items with M % 16 == 0 go instead to one launch of the K-chunked streaming MMQ (a K over
 * 4096 in ranges of 4096 whose fp32 partials a second launch sums), each item bit-identical to
 * its own gq_mmq_prepared_ex (which takes the same kernel for K <= 4096; GQ_KSTREAM=1 for
 * longer K); GQ_KSTREAM=0 keeps every item on the streaming GEMM.  workspace: the K-range and
 * split-K partials, >= gq_mmq_grouped_prepared_workspace_size() bytes (0 when nothing splits:
 * NULL allowed).  GQ_EUNSUPPORTED (nothing launched) for N < 5, more than 16 items, K % 256 != 0
 * or >= 2 GiB in one item: call gq_mmq_prepared_ex per item then.  No host sync.
 */
typedef struct gq_gemm_item {
    gq_type type;
    const void *A;
    const void *ws;
    void *C;
    int64_t ldc;
    int64_t M, K;
} gq_gemm_item;
size_t gq_mmq_grouped_prepared_workspace_size(gq_act act, const gq_gemm_item *items, int n, int64_t N);
int gq_mmq_grouped_prepared(gq_act act, const gq_gemm_item *items, int n, int64_t N, void *workspace,
                            size_t workspace_bytes, void *stream);

/* Text of the last error on this thread ("" if none). */
const char *gq_last_error(void);

/* Library ABI version (major * 100 + minor).  103: gq_gemm_item, gq_mmq_grouped_prepared[_workspace_size],
 * gq_debug_route, and larger workspace sizes for the GEMM routes (round 4).  104: gq_mmq_grouped[_ex]
 * takes 5..32 tokens (the K-chunked streaming MMQ; round 5).  105: GEMM workspace sizes grow by the
 * in-launch split-K combine's flag words (opt-in GQ_RGEMM_ILC=1: the resident and streaming GEMMs
 * sum their split-K partials inside their own launch; measured slower, off by default) and
 * gq_debug_sync_timeouts (round 6). */
int gq_version(void);

/*
 * Debug / tuning only (no counterpart in the reference; not for production callers).  The
 * library reads its GQ_* tuning variables from the environment ONCE, at first use; this entry
 * overrides one of them by name (e.g. "GQ_GEMM_SPLITS", "GQ_RGEMM_ILC", "GQ_RGEMM_ESTORE") for later calls in the
 * process.  Values no kernel is instantiated for are rejected (GQ_EINVAL).  Not thread-safe
 * against calls running concurrently on other threads.  reset: back to the environment's values.
 */
int gq_debug_set_tuning(const char *key, long long value);
void gq_debug_reset_tuning(void);
/* The kernel(s) a gq_mmq_ex call (prepared = 0) or a gq_mmq_prepared_ex call (prepared = 1) of
 * this shape would launch under the current tuning ("none" for an invalid shape): what bench.py
 * names as its roofline kernel.  Split-K reduce kernels are listed whether or not the plan
 * splits. */
const char *gq_debug_route(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K, int prepared);
/* The one-launch decode's plan for a call, host only (no device is touched once GQ_CUS is set): what
 * tests/decode_cases.py builds its case table from.  family: 0 gq_mmq_ex's decode, 1 gq_mmq_id,
 * 2 gq_mmq_id_glu, 3 gq_mmq_glu -- items[0]'s type, M and K with n = 1, N the tokens (families 1, 2:
 * the N*S pairs) -- or 4 gq_mmq_grouped_ex on the n items.  Pointers and strides in the items are not
 * read.  Returns how many entries the call's launches have -- one per (item, token group), at most
 * max_out of them written to out -- or 0 when that entry point would not take its one-launch decode
 * for the call under the current tuning.
 *   nt, itc, img, fp8 : the kernel: token tile, cached activation chunks, Q6_K's aligned ring, fp8 form
 *   lds_split         : the tile was cut to fit LDS (never set in an accepted plan)
 *   nseg, G, lp2      : segments per row, rows per task, log2 of the lanes per row
 *   grid, ngroups     : workgroups (families 1, 2: per pair; 4: the item's share) and the row groups
 *                       (rows when nseg > 1) they share, 8 waves each
 *   stash_rows        : families 2, 3: uint16 entries of a wave's g stash per token
 *   tokens            : tokens in this entry's token group
 *   set, item         : family 4: the launch's case set and the entry's item
 *   lds               : the launch's dynamic LDS bytes
 * Debug entry points: they do not move gq_version. */
typedef struct gq_decode_plan {
    int32_t nt, itc, img, fp8, lds_split, nseg, G, lp2, grid, ngroups, stash_rows, tokens, set, item, lds;
} gq_decode_plan;
int gq_debug_decode_plan(int family, gq_act act, const gq_group_item *items, int n, int64_t N, gq_decode_plan *out,
                         int max_out);
/* The most cached chunks (itc) a decode kernel of the family exists for at (type, token tile nt in
 * 1, 2, 4, fp8 form), or -1 when it has none; family as above, set: family 4's case set (0..4). */
int gq_debug_decode_cap(int family, int set, gq_type t, int nt, int fp8);
/* The GEMM kernels a call would launch under the current tuning, host only (no device is touched once
 * GQ_CUS is set): what tests/gemm_cases.py builds its case table from.  entry: 0 gq_mmq_ex, 1
 * gq_mmq_prepared_ex, 2 gq_mmq_id_sorted (N tokens x S slots on E experts) -- items[0]'s type, M and K
 * with n = 1 --, 3 gq_mmq_grouped_prepared, 4 gq_mmq_grouped_ex at 5..32 tokens (fp8: 3..32) on the n
 * items; E and S are read by entry 2 alone.  Pointers and strides in the items are not read: the call
 * is taken as contiguous and aligned, as gq_debug_route takes it.  Returns how many entries the call's
 * launches have, at most max_out of them written to out: one per launched kernel in launch order (a
 * raw call's act_quant launch is not listed), sgemm_grouped_kernel one per item of its launch; 0 when
 * the call takes no kernel of mmq_rgemm / mmq_gemm / mmq_skinny / mmq_kstream (decode, GEMV, the
 * library GEMM, a refused shape).  Fields that do not apply to a kernel are 0.
 *   kernel            : GQ_GK_*
 *   fmt               : the weight type (-1: a launch of several items)
 *   nb, rg, am, nl, aq, es, set, cwm : the template parameters -- token tiles of 16 (skinny, kstream: NT, NB), row
 *                       groups, activation form, loader waves, in-kernel quantization (1 q8_1, 2 fp8),
 *                       early store, the grouped case set, kstream's chunk form
 *   splits, chunks_per_split, pf16 : the K splits, super-blocks per split (the longest), fp16 partials
 *   ilc               : the split-K sum inside the launch AS THE PLAN DECIDES IT.  The launchers also ask
 *                       the runtime how many workgroups of the kernel a CU admits and take the
 *                       two-launch form when the grid would not be resident; that check needs the
 *                       device and is not part of this answer
 *   order             : sgemm_kernel's grid order (0 3-D grid, 1 in-launch sum, 2 split-major)
 *   full, streamk     : sgemm_full_body runs (Q4_K, 16/32-token tiles); the stream-K unit split
 *   tiles_m, tiles_n, blocks : row tiles (skinny: units, kstream: 16-row items), token tiles (sorted:
 *                       table entries), workgroups of the launch
 *   item              : the entry's index in items (-1: a launch of several)
 *   rows, toks        : rows and tokens of this launch (the chunked kernels: the chunk's)
 *   partial_bytes     : the partials this launch's plan needs (the ABI's workspace sizes cover them)
 * A debug entry point: it does not move gq_version. */
enum {
    GQ_GK_NONE = 0, GQ_GK_RGEMM, GQ_GK_SGEMM, GQ_GK_SGEMM_ID, GQ_GK_SGEMM_GROUPED, GQ_GK_REDUCE_GROUPED, GQ_GK_GEMM,
    GQ_GK_GEMM_REDUCE_F16, GQ_GK_GEMM_REDUCE, GQ_GK_SKINNY, GQ_GK_KSTREAM, GQ_GK_KSTREAM_REDUCE
};
typedef struct gq_gemm_plan {
    int32_t kernel, fmt, nb, rg, am, nl, aq, es, set, cwm;
    int32_t splits, chunks_per_split, pf16, ilc, order, full, streamk;
    int32_t tiles_m, tiles_n, blocks, item;
    int64_t rows, toks;
    uint64_t partial_bytes;
} gq_gemm_plan;
int gq_debug_gemm_plan(int entry, gq_act act, const gq_group_item *items, int n, int64_t N, int64_t E, int64_t S,
                       gq_gemm_plan *out, int max_out);
/* How many synchronisation waits inside a kernel gave up since the library was loaded: the
 * resident GEMM's in-launch split-K combine (only possible when another kernel holds CUs its grid
 * needed) and the K-chunked stream's cross-wave hand-off.  A wait gives up after a bounded spin
 * (wrong bits, never a hang).  Tests assert it stays 0. */
unsigned int gq_debug_sync_timeouts(void);

#ifdef __cplusplus
}
#endif

#endif /* GGUF_MMQ_H */

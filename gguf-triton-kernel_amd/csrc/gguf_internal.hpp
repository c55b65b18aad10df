// gguf_internal.hpp -- launchers shared between the kernel translation units and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gq {

// Tuning overrides of the measured defaults.  Read ONCE per process from GQ_* environment
// variables (gq_capi.hip, std::call_once) -- the launch path never calls getenv -- and changed
// at run time only through the debug entry point gq_debug_set_tuning (tests, A/B tools; not
// thread-safe against concurrent launches).  0 / -1 = "the default the code measured".
struct Tuning {
    long long blas_min_tokens = 768;          // GQ_BLAS_MIN_TOKENS: library GEMM from this many tokens (<= 0: never)
    long long gemm_max_bytes = 1LL << 31;     // GQ_GEMM_MAX_BYTES: weight / activation bytes per GEMM launch
    int gemm_i8 = 0;                          // GQ_GEMM_I8: Q8_0 int8-MFMA form
    int fused_decode = 1;                     // GQ_NO_FUSED_DECODE=1 -> 0
    int decode_f8_itc = 1;                    // GQ_DECODE_F8_ITC: fp8 decode keeps x~ in registers at one token
    int decode_q6_img = -1;                   // GQ_DECODE_Q6_IMG: Q6_K aligned ring image (-1: K <= 4096)
    int gemm_aq = 1;                          // GQ_GEMM_AQ: in-kernel quantization of 16/32-token tiles
    int gemm_rg = 0;                          // GQ_GEMM_RG: 1 or 2 (0: auto)
    long long gemm_splits = 0;                // GQ_GEMM_SPLITS: split-K factor (0: auto)
    int gemm_partial_f32 = 0;                 // GQ_GEMM_PARTIAL=f32
    int skinny = -1;                          // GQ_SKINNY: 5..32-token kernel (-1 auto, 0 off, 1 every 1..32)
    int skinny_rg = 0;                        // GQ_SKINNY_RG: fragments per workgroup, 1..4 (0: auto)
    int rgemm = -1;                           // GQ_RGEMM: resident-split GEMM -1 auto / 0 off / 1 wherever it applies
    int sgemm = -1;                           // GQ_SGEMM: streaming 256-row GEMM -1 auto / 0 off / 1 wherever it applies
    int sgemm_splits = 0;                     // GQ_SGEMM_SPLITS (0: auto)
    int sgemm_streamk = -1;                   // GQ_SGEMM_STREAMK: stream-K unit split of the auto plan: 1 every
                                              // streaming GEMM, 0 none, -1 the grouped plans (the measured gain)
    int rgemm_ilc = 0;                        // GQ_RGEMM_ILC: split-K sums inside the GEMM launch (measured slower: opt-in)
    int rgemm_estore = -1;                    // GQ_RGEMM_ESTORE: resident GEMM's partial stores under its second half
                                              // multiply: 1 every tile that has the form, 0 none, -1 where measured faster
    int sgemm_full = -1;                      // GQ_SGEMM_FULL: Q4_K 16/32-token tiles stream whole super-blocks:
                                              // 1 every streaming GEMM, 0 none, -1 single matrices (measured gain)
    int kstream = -1;                         // GQ_KSTREAM: K-chunked streaming MMQ -1 auto / 0 off / 1 wherever it applies
    int cus = 0;                              // GQ_CUS: compute units to plan for (0: the device's count)
    int ablate = 0;                           // GQ_ABLATE (GQ_ABLATION diagnostic builds only)
};
const Tuning &tuning();
// key = the environment variable's name ("GQ_GEMM_SPLITS", ...); value validated (an override
// that no kernel is instantiated for is rejected).  Returns 0, or -1 for an unknown key or a
// value out of range.  reset: back to the environment's values.
int set_tuning(const char *key, long long value);
void reset_tuning();
// compute units of the current device (hipDeviceAttributeMultiprocessorCount, queried once per
// device), or the GQ_CUS override: every "one round of the chip" plan sizes its grid by it
int num_cus();

enum ActMode : int { ACT_AOS = 0, ACT_SOA = 1, ACT_DEQ = 2, ACT_I8 = 3, ACT_F8 = 4, ACT_F8DEQ = 5 };
// Activation form the MFMA GEMM reads (mmq_gemm.hip): fp16 x~ (q8_1's, or the fp8 variant's
// widened e4m3 codes) or q8_1 codes (Q8_0 int8 MFMA).
enum ActForm : int { AF_F16 = 0, AF_I8 = 1 };

// Activation quantizer (act_quant.hip).  AOS: out0 = q8_1 bytes.  SOA: out0 = int8 codes
// [rows][K], out1 = float d [rows][K/32], out2 = float s [rows][K/32].  DEQ: out0 = fp16 x~.
// I8: out0 = int8 codes [rows][K], out1 = float d [K/32][(rows + 3) & ~3] (block-major).
// F8 (the fp8 activation variant, not q8_1): out0 = OCP e4m3 codes [rows][K], each 4-element
// group stored (0,2,1,3); out1 = float 2^e [K/32][(rows + 3) & ~3], e the smallest integer with
// max|x| <= 448 * 2^e over the block (2^0 for an all-zero block); code = e4m3(x / 2^e), RNE.
// F8DEQ: out0 = fp16 code * 2^e [rows][K] in the DEQ layout (the fp8 variant's GEMM input).
// Weight quantizers on the device (quant_device.hip): kind 0 Q8_0 (fp16 in), 1 Q4_K (fp32),
// 2 Q6_K (fp32), 3 Q8_1 (fp16), 4 Q4_0 (fp32); the host producers' bytes.
hipError_t launch_quant_blocks(int kind, const void *x, void *y, int64_t nblocks, hipStream_t s);

hipError_t launch_act_quant(int mode, const uint16_t *X, int64_t ldx, int64_t rows, int64_t K, void *out0,
                            void *out1, void *out2, hipStream_t s);
// The DEQ form of up to kMaxDeqSegs tensors in one launch (wg0 is set by the launcher),
// bit-identical to launch_act_quant(ACT_DEQ, ...) per tensor.
constexpr int kMaxDeqSegs = 8;
struct DeqSeg {
    const uint16_t *X;
    int64_t ldx, rows, K;
    uint16_t *xdeq;
    int64_t wg0;
};
hipError_t launch_act_quant_deq_grouped(const DeqSeg *segs, int n, hipStream_t s, int mode = ACT_DEQ); // or ACT_F8DEQ

// Residual add + RMSNorm (rmsnorm.hip), one workgroup per row: h = R ? fp16(x + r) : x,
// y = fp16((h * 1/sqrtf(mean(h^2) + eps)) * w).  Every output is optional: H and Y (fp16, rows ldh /
// ldy apart) and act_quant's q8_1 forms of y, rows K apart -- xq + xd + xs (SOA; xraw: the fp16 copy
// beside it) or xdeq (DEQ), never both.  N < 2^31, K % 32 == 0.
constexpr int kNormChunk = 2048;   // elements a workgroup covers per step (256 lanes x 8)
constexpr int kNormRegChunks = 8;  // rows up to this many chunks stay in registers; longer: read twice
struct NormArgs {
    const uint16_t *X, *R;
    uint16_t *H, *Y;
    const float *w;
    float eps;
    int64_t K, ldx, ldr, ldh, ldy;
    int8_t *xq;
    float *xd, *xs;
    uint16_t *xdeq, *xraw;
};
hipError_t launch_rmsnorm(const NormArgs &a, int64_t N, hipStream_t s);

// Decode-shaped GEMV (mmq_gemv.hip): C[t][m] for t < N_tok <= 8 from SOA activations.
hipError_t launch_gemv(int fmt, const uint8_t *A, const int8_t *xq, const float *xd, const float *xs, uint16_t *C,
                       int64_t M, int64_t N, int64_t K, int64_t ldc, hipStream_t s);

// Streaming decode (mmq_decode.hip): q8_1 quantization of the N <= 8 tokens in LDS + the
// weight stream, one launch.  decode_fused_ok() says whether the LDS image fits (else:
// act_quant + launch_gemv).  fp8: the fp8 activation variant's form (e4m3-quantized x~ in LDS,
// fp16 dot products).
bool decode_fused_ok(int fmt, int64_t N, int64_t K, bool fp8 = false);
hipError_t launch_decode_fused(int fmt, const uint8_t *A, const uint16_t *X, int64_t ldx, uint16_t *C, int64_t M,
                               int64_t N, int64_t K, int64_t ldc, hipStream_t s, bool fp8 = false);

// 16-token groups per workgroup tile for N tokens (a sorted expert GEMM: the mean per expert):
// every MFMA GEMM plan's nb -- 16-, 32-, 64- or 128-token tiles
constexpr int pick_nb(int64_t N) { return N > 64 ? 8 : (N > 32 ? 4 : (N > 16 ? 2 : 1)); }

// Batched GEMM on fp16 MFMA (mmq_gemm.hip): C[t][m] from the dequantized activation x~.
struct GemmPlan {
    int nb = 8;                // 16-token groups per workgroup (tile = 16*nb tokens)
    int rg = 2;                // 16-row groups per wave (8 waves: tile = 128*rg weight rows)
    int splits = 1;            // split-K factor (grid.z)
    int chunks_per_split = 1;  // 256-wide K stages (super-blocks) per split
    int act = AF_F16;          // activation form (AF_I8: Q8_0 only)
    int loaders = 0;           // 4: four dedicated DMA-issuing waves beside the 8 multiplying ones
    int pf16 = 0;              // split-K partials stored as fp16 (else fp32)
    int aq = 0;                // activations quantized in-kernel from raw fp16 (GemmAct::xraw)
    size_t partial_bytes = 0;  // fp32 partial slabs needed when splits > 1
};
// Activations as the GEMM reads them: fp16 x~ (act_quant DEQ) or, for the code forms, codes +
// block-major fp32 scales (act_quant I8 / F8).
struct GemmAct {
    const uint16_t *xdeq = nullptr;
    const int8_t *xq = nullptr;
    const float *xd = nullptr;
    int64_t ldd = 0; // row length of the block-major scale array (all the call's tokens)
    const uint16_t *xraw = nullptr; // aq: the fp16 activations themselves, rows ldx apart
    int64_t ldx = 0;
};
// plan.aq is allowed (in-kernel q8_1 of a 16/32-token tile's split, GemmPlan::aq)
bool gemm_aq_ok(const GemmPlan &p);
// The MFMA GEMM needs K in whole 256-element stages (always true for Q4_K/Q6_K).
bool gemm_supported(int fmt, int64_t K);
// act: the activation form (AF_I8 is honoured for Q8_0 only).
GemmPlan plan_gemm(int fmt, int64_t M, int64_t N, int64_t K, int act = AF_F16);
hipError_t launch_gemm(int fmt, const uint8_t *A, const GemmAct &x, uint16_t *C, float *partials,
                       const GemmPlan &plan, int64_t M, int64_t N, int64_t K, int64_t ldc, hipStream_t s);

// The split-K sum of the fp16 partials gemm_kernel (and rgemm_kernel, sgemm_kernel) write: tiles of
// 16*8*rg rows x 16*nb tokens, S splits (mmq_gemm.hip gemm_reduce_f16_kernel; the partial's layout:
// gguf_partial.hpp).
int gemm_reduce_blocks(int tiles_x, int tiles_y, int rg, int nb); // its workgroups
hipError_t launch_gemm_reduce_f16(int nb, int rg, const uint16_t *P, uint16_t *C, int64_t M, int64_t N, int64_t ldc,
                                  int S, int tiles_x, int tiles_y, hipStream_t s);

// Resident-split GEMM (mmq_rgemm.hip): 256 rows x 16*nb tokens x one super-block per workgroup,
// the split's weights and activations loaded once into LDS; split-K over every super-block
// (fp16 partials + launch_gemm_reduce_f16).  aq: 0 prepared x~ (X = [N][K] DEQ / F8DEQ form),
// 1 raw fp16 activations (X rows ldx apart) q8_1-quantized in-kernel, 2 raw, fp8-quantized.
struct RGemmPlan {
    bool ok = false;
    int nb = 8, tiles_m = 0, tiles_n = 0, splits = 1;
    size_t partial_bytes = 0;
};

RGemmPlan plan_rgemm(int64_t M, int64_t N, int64_t K);
// the split-K partials summed inside the launch (no reduce launch): plans whose grid the chip holds
bool rgemm_ilc(int fmt, const RGemmPlan &p);
// whether the resident GEMM at nb token tiles (RGemmPlan::nb) runs its early-store form (GQ_RGEMM_ESTORE)
bool rgemm_estore(int nb);
// in-launch combine polls that gave up since the library loaded (0 unless a grid was not resident)
unsigned int ilc_timeouts();
// the K-chunked stream's cross-wave hand-off waits that gave up (0 unless broken)
unsigned int kstream_timeouts();
// resident workgroups one CU holds at once (LDS-bound: Q4_K at 16 tokens 3, at 32 two, else one);
// 0 for a type without a resident form or an nb that is not pick_nb's
int rgemm_per_cu(int fmt, int nb);
// launch_rgemm takes the call: a plan, and 16-byte activation rows where the kernel quantizes them
bool rgemm_call_ok(int aq, int64_t ldx, const RGemmPlan &p);
hipError_t launch_rgemm(int fmt, int aq, const uint8_t *A, const uint16_t *X, int64_t ldx, uint16_t *C, void *partials,
                        const RGemmPlan &p, int64_t M, int64_t N, int64_t K, int64_t ldc, hipStream_t s);
// Streaming form (mmq_rgemm.hip sgemm_kernel): the same tile over K splits of several
// super-blocks, half-super-block stages through an LDS ring; prepared x~ only (X = [N][K]).
// splits <= 0: as many as keep the grid within one round of the chip.
RGemmPlan plan_sgemm(int64_t M, int64_t N, int64_t K, int splits);
// its split-K sum inside the launch (as rgemm_ilc; the streaming kernel holds one workgroup per CU)
bool sgemm_ilc(const RGemmPlan &p);
hipError_t launch_sgemm(int fmt, const uint8_t *A, const uint16_t *X, uint16_t *C, void *partials, const RGemmPlan &p,
                        int64_t M, int64_t N, int64_t K, int64_t ldc, hipStream_t s);

// Several streaming GEMMs in one launch (+ one grouped split-K reduce), at most 16 items sharing
// the token count N; X = each item's prepared x~ ([N][K]).  The plan spreads the super-blocks
// over one round of the chip: the fewest per workgroup that fit, every item split accordingly
// (splits > 0: that split factor for every item, as plan_sgemm's).
struct SGroupItem {
    int fmt;
    const uint8_t *A;
    const uint16_t *X;
    uint16_t *C;
    int64_t ldc, M, K;
};
struct SGroupPlan {
    bool ok = false;
    int nb = 8, tiles_n = 1, blocks = 0;
    int tiles_m[16] = {}, splits[16] = {}, wg0[16] = {};
    bool streamk = false;  // (tile, super-block) units spread evenly over the workgroups (auto splits)
    int U = 0;             // stream-K: total cost of the units (each part's units cost[i]); blocks = the workgroups
    int ustart[16] = {}, scap[16] = {};
    int cost[16] = {}, cstart[16] = {}; // stream-K: a part's per-unit cost, the cost before its first unit
    size_t poff[16] = {};
    size_t foff[16] = {}, noff[16] = {}; // stream-K split parts: the in-launch combine's flags, nonces
    size_t partial_bytes = 0;
};
SGroupPlan plan_sgemm_grouped(const SGroupItem *items, int n, int64_t N, int splits);
hipError_t launch_sgemm_grouped(const SGroupItem *items, int n, int64_t N, const SGroupPlan &g, void *partials,
                                hipStream_t s);

// Grouped decode (mmq_decode.hip): several matrices -- each its own type, activations (N x K
// fp16, row stride ldx) and output (N x M, stride ldc) -- in one launch per token tile, the
// chip's waves split by weight bytes; each matrix's rows come out bit-identical to its own
// launch_decode_fused.  N <= 4, every item decode_fused_ok, at most 16 (item, token group) parts.
struct DecodeItem {
    int fmt;
    const uint8_t *A;
    const uint16_t *X;
    int64_t ldx;
    uint16_t *C;
    int64_t ldc;
    int64_t M, K;
};
bool decode_grouped_ok(const DecodeItem *items, int n, int64_t N, bool fp8 = false);
hipError_t launch_decode_grouped(const DecodeItem *items, int n, int64_t N, hipStream_t s, bool fp8 = false);

// Expert-indexed decode (mmq_decode.hip; llama.cpp's mul_mat_id at decode): pairs = N*S (token,
// slot) pairs, pair p = n*S + s multiplying expert ids[p] (int32 in device memory, read by the
// kernel) of the E packed M x K matrices at A by the fp16 row B + n*ldb + s*ldb_slot into
// C + p*ldc; each pair's M outputs are the bits of its own one-token launch_decode_fused, an id
// outside [0, E) gives M zeros.  One launch, q8_1 activations only, no workspace.
// kMaxIdPairs: every pair streams its expert's weights on its own share of the chip, so two pairs
// that pick one expert read it twice; up to 8 tokens x top-8 that costs less than sorting the
// pairs would, beyond it pairs sharing an expert should share one weight stream (a sorted GEMM,
// not this kernel).  decode_id_ok: the launch's plan (mmq_decode.hip plan_id) succeeds -- pairs <=
// kMaxIdPairs, the one-token fused decode fits (decode_fused_ok(fmt, 1, K)), one expert is < 2 GiB
// (32-bit buffer offsets; the whole tensor may be larger) and the pairs' share of the chip picks the
// one-token launch's kernel -- else the caller falls back.
constexpr int kMaxIdPairs = 64;
bool decode_id_ok(int fmt, int64_t M, int64_t pairs, int64_t K);
hipError_t launch_decode_id(int fmt, const uint8_t *A, const int32_t *ids, const uint16_t *B, uint16_t *C, int64_t E,
                            int64_t M, int64_t N, int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc,
                            hipStream_t s);

// Expert-indexed gate / up with SwiGLU (mmq_decode.hip; gq_mmq_id_glu): launch_decode_id's pairs,
// grid and geometry on two expert tensors of one type and shape, one launch, one activation
// prologue per workgroup.  With g and u the fp16 values launch_decode_id writes for a pair's row
// from A_gate and A_up, H + p*ldh holds fp16(g / (1 + expf(-g)) * u), evaluated in fp32.
// decode_id_glu_ok: decode_id_ok, and the waves' stash of g values fits the launch's LDS.
bool decode_id_glu_ok(int fmt, int64_t M, int64_t pairs, int64_t K);
hipError_t launch_decode_id_glu(int fmt, const uint8_t *A_gate, const uint8_t *A_up, const int32_t *ids, const uint16_t *B,
                                uint16_t *H, int64_t E, int64_t M, int64_t N, int64_t S, int64_t K, int64_t ldb,
                                int64_t ldb_slot, int64_t ldh, hipStream_t s);

// Dense gate / up with SwiGLU (mmq_decode.hip; gq_mmq_glu): launch_decode_fused's grid, geometry and
// token tile on two matrices of one type and shape, one launch, one activation prologue per
// workgroup.  With g and u the fp16 values launch_decode_fused writes at this N from A_gate and
// A_up, H[n*ldh + m] holds fp16(g / (1 + expf(-g)) * u), evaluated in fp32.
// decode_glu_ok: N <= kGluMaxTokens, decode_fused_ok, one matrix < 2 GiB, a kernel exists for the
// pick's cached chunks (the instantiations that would spill are left out) and the waves' stash of
// g values fits the launch's LDS without costing a workgroup per CU.  The caller asks the call's
// route first (gq_capi.hip plan_call: the one-launch decode).
constexpr int kGluMaxTokens = 4;
bool decode_glu_ok(int fmt, int64_t M, int64_t N, int64_t K);
hipError_t launch_decode_glu(int fmt, const uint8_t *A_gate, const uint8_t *A_up, const uint16_t *X, int64_t ldx,
                             uint16_t *H, int64_t M, int64_t N, int64_t K, int64_t ldh, hipStream_t s);

// The decode plans as data (mmq_decode.hip; gq_debug_decode_plan, gq_debug_decode_cap): host only.
// decode_plan_info: the launches the family's launcher would make, one entry per (launch part, token
// group), from the launcher's own planning functions; returns their count (0: the family has no
// one-launch decode for the call), filling at most max_out.  DF_DENSE launch_decode_fused, DF_ID /
// DF_ID_GLU launch_decode_id[_glu] (N: the pairs), DF_GLU launch_decode_glu: items[0]'s fmt, M, K,
// n == 1; DF_GROUPED launch_decode_grouped on the n items.  Pointers and strides are not read.
// decode_itc_cap: the most cached chunks a kernel of the family exists for at (type, token tile,
// form) -- set: the grouped kernel's case set -- or -1 when there is none at all.
enum DecodeFamily : int { DF_DENSE = 0, DF_ID = 1, DF_ID_GLU = 2, DF_GLU = 3, DF_GROUPED = 4 };
struct DecodePlanInfo { // (gq_decode_plan's fields, in its order)
    int nt, itc, img, fp8, lds_split, nseg, G, lp2, grid, ngroups, stash_rows, tokens, set, item, lds;
};
int decode_plan_info(int family, const DecodeItem *items, int n, int64_t N, bool fp8, DecodePlanInfo *out, int max_out);
int decode_itc_cap(int family, int set, int fmt, int nt, bool fp8);

// Router-weighted sum over slots (moe_combine.hip; gq_moe_combine): Y[n][m] = fp16(sum_s W[n*S+s] *
// D[(n*S+s)*ldd + m]), the products and sums in fp32 in slot order, uncontracted; no atomics.
hipError_t launch_moe_combine(const uint16_t *D, const void *W, bool w_f32, uint16_t *Y, int64_t N, int64_t S, int64_t M,
                              int64_t ldd, int64_t ldy, hipStream_t s);
// The same with a shared expert's term after the slots (gq_moe_combine_shared): acc = acc + dsh, or
// acc + gate[n] * dsh (uncontracted) when gate is not null; Dsh fp16, token n's M values at n*ldsh.
hipError_t launch_moe_combine_shared(const uint16_t *D, const void *W, bool w_f32, const uint16_t *Dsh, int64_t ldsh,
                                     const float *gate, uint16_t *Y, int64_t N, int64_t S, int64_t M, int64_t ldd,
                                     int64_t ldy, hipStream_t s);

// The router (moe_route.hip; gq_moe_topk, gq_moe_route), one launch each.
//   launch_moe_topk: token n's S experts of largest key out of logits[n*ldl + e] (descending, the
//     lower index first on ties, NaN last; always S distinct ids in [0, E)) into ids[n*S + s], and
//     their weights (softmax over all E or sigmoid, optionally renormalised over the S, times
//     scale) into W[n*S + s]; one wave per token, any N.  moe_topk_ok: 1 <= S <= E <=
//     kMaxSortExperts and S <= kMaxIdPairs.
//   launch_moe_logits: L[n*ldl + e] = sum_k X[n*ldx + k] * Wr[e*H + k] in fp32, one workgroup per
//     expert row, the summation order of an (n, e) fixed whatever N is.  moe_logits_ok: N <=
//     kMaxRouteTokens and H % 32 == 0.
constexpr int kMaxRouteTokens = 64;
bool moe_topk_ok(int64_t E, int64_t S);
bool moe_logits_ok(int64_t N, int64_t H);
hipError_t launch_moe_topk(const float *logits, int64_t ldl, const float *bias, int func, bool norm, float scale, int32_t *ids,
                           void *W, bool w_f32, int64_t N, int64_t E, int64_t S, hipStream_t s);
hipError_t launch_moe_logits(const void *Wr, bool wr_f16, const uint16_t *X, int64_t ldx, float *L, int64_t ldl, int64_t N,
                             int64_t E, int64_t H, hipStream_t s);

// Sorted expert GEMM (gq_mmq_id_sorted; any pair count): three launches whose grids depend on
// host-known sizes only.
//   launch_id_sort (mmq_idsort.hip): one workgroup; perm[P] = the pair indices grouped by expert
//     (ascending inside a group, out-of-range ids last), hdr = {T, nvalid, 0, 0}, table[T] =
//     {expert, first sorted row, rows <= 16*nb, 0} per (expert, token tile).
//   launch_act_quant_gather (act_quant.hip): sorted row r = act_quant's DEQ x~ of pair perm[r]'s
//     row B + n*ldb + s*ldb_slot (the bytes gq_act_prepare writes for that row); the M outputs of
//     the out-of-range pairs (rows >= nvalid) zeroed in C.
//   launch_sgemm_id (mmq_rgemm.hip): tiles_m x t_max workgroups, workgroup (x, t < T) the
//     streaming GEMM body on table entry t over the whole K, sorted row r stored to
//     C + perm[row0 + r]*ldc; t >= T returns at once.
// t_max = min(E, P) + P / (16*nb) bounds sum_e ceil(c_e / (16*nb)) for any ids (every expert with
// pairs has at most one partial tile, and the full tiles hold 16*nb pairs each).
constexpr int kMaxSortExperts = 1024, kMaxSortPairs = 65536;
struct SortedPlan {
    bool ok = false;
    int nb = 1, tiles_m = 0, t_max = 0;
    size_t perm_off = 0, hdr_off = 0, table_off = 0, bytes = 0; // from the 16-byte aligned workspace (x~ at 0)
};
SortedPlan plan_sgemm_id(int64_t E, int64_t M, int64_t P, int64_t K);
hipError_t launch_id_sort(const int32_t *ids, int64_t P, int64_t E, int nb, int32_t *perm, int32_t *hdr, int32_t *table,
                          hipStream_t s);
hipError_t launch_act_quant_gather(const uint16_t *B, int64_t ldb, int64_t ldb_slot, int64_t S, const int32_t *perm,
                                   const int32_t *hdr, int64_t P, int64_t K, uint16_t *xdeq, uint16_t *C, int64_t M,
                                   int64_t ldc, hipStream_t s);
hipError_t launch_sgemm_id(int fmt, const uint8_t *A, const uint16_t *X, uint16_t *C, const int32_t *perm,
                           const int32_t *hdr, const int32_t *table, const SortedPlan &p, int64_t M, int64_t K, int64_t ldc,
                           hipStream_t s);

// K-chunked streaming MMQ (mmq_kstream.hip, 5..32 tokens): x~ in VGPRs (each of a workgroup's
// 8 waves one K chunk), weights streamed per wave through private LDS rings, the waves' tiles
// summed in LDS: one launch, no partials for K <= 4096.  A longer K is cut into ranges of 16
// super-blocks whose fp32 partial tiles (kstream_partial_bytes of workspace) one small launch
// sums in range order.  Up to kKMaxParts matrices x ranges (own type, activations, output; the
// same N) in one launch, workgroups apportioned by weight bytes; a matrix's bits do not depend on
// the launch it is in.  aq: 0 prepared x~ (X = [N][K], ldx = K, act_quant DEQ / F8DEQ), 1 raw fp16
// q8_1-quantized in-kernel, 2 raw fp16 with the fp8 variant's quantization.
// kstream_ok: K % 256 == 0, M % 16 == 0, < 2 GiB of weights.
constexpr int kKMaxParts = 24;
struct KItem {
    int fmt;
    const uint8_t *A;
    const uint16_t *X;
    int64_t ldx;
    uint16_t *C;
    int64_t ldc, M, K;
};
int kstream_splits(int64_t K);
int kstream_cw(int64_t N, int64_t K);
bool kstream_ok(int fmt, int64_t M, int64_t N, int64_t K);
size_t kstream_partial_bytes(const KItem *items, int n, int64_t N);
hipError_t launch_kstream(const KItem *items, int n, int64_t N, int aq, void *partials, hipStream_t s);

// Skinny-token MMQ (mmq_skinny.hip, 1..32 tokens, K % 256 == 0): 16*rg rows x 16*nb tokens per
// workgroup, K split over its 8 waves (8/nb ranges x nb token tiles), weights and activations
// (fp16 x~, DEQ form) streamed into registers through a d-deep super-block ring, one launch, no
// partials.  rg in 1..4, d = 2.
struct SkinnyPlan {
    int rg = 1, nb = 1, d = 3;
};
SkinnyPlan plan_skinny(int fmt, int64_t M, int64_t N, int64_t K, int rg, int d);
bool skinny_call_ok(int fmt, const SkinnyPlan &plan, int64_t M, int64_t N, int64_t K); // launch_skinny takes the call
hipError_t launch_skinny(int fmt, const uint8_t *A, const uint16_t *X, uint16_t *C, const SkinnyPlan &plan, int64_t M,
                         int64_t N, int64_t K, int64_t ldc, hipStream_t s);

// The GEMM plans as data (gq_debug_gemm_plan): host only, one entry per kernel a launcher would
// launch, written by the launcher's own deciding functions (each *_plan_info below sits beside its
// launcher and calls what the launcher calls).  Fields that do not apply to a kernel stay 0.  ilc is
// the plan's answer: the launchers also ask the runtime's occupancy for the kernel (a device query)
// and take the two-launch form when the grid would not be resident; that check is not in here.
enum GemmKernelId : int {
    GK_NONE = 0, GK_RGEMM, GK_SGEMM, GK_SGEMM_ID, GK_SGEMM_GROUPED, GK_REDUCE_GROUPED, GK_GEMM, GK_GEMM_REDUCE_F16,
    GK_GEMM_REDUCE, GK_SKINNY, GK_KSTREAM, GK_KSTREAM_REDUCE
};
struct GemmPlanInfo { // (gq_gemm_plan's fields, in its order)
    int kernel, fmt, nb, rg, am, nl, aq, es, set, cwm;                    // the kernel and its template parameters
    int splits, chunks_per_split, pf16, ilc, order, full, streamk;        // its run-time form
    int tiles_m, tiles_n, blocks, item;                                   // its geometry; item: the list entry (-1: several)
    int64_t rows, toks;                                                   // rows and tokens of this launch
    uint64_t partial_bytes;                                               // partials the launch's plan needs
};
// appends to out[at..max_out) and returns the new count (entries past max_out are counted, not written)
int rgemm_plan_info(int fmt, int aq, int64_t ldx, const RGemmPlan &p, int64_t M, int64_t N, int64_t K, GemmPlanInfo *out, int at, int max_out);
int sgemm_plan_info(int fmt, const RGemmPlan &p, int64_t M, int64_t N, int64_t K, GemmPlanInfo *out, int at, int max_out);
int sgemm_id_plan_info(int fmt, const SortedPlan &p, int64_t M, int64_t K, GemmPlanInfo *out, int at, int max_out);
int sgemm_grouped_plan_info(const SGroupItem *items, int n, int64_t N, const SGroupPlan &g, const int *item_ids,
                            GemmPlanInfo *out, int at, int max_out);
int gemm_plan_info(int fmt, const GemmPlan &p, int64_t M, int64_t N, int64_t K, GemmPlanInfo *out, int at, int max_out);
int skinny_plan_info(int fmt, const SkinnyPlan &p, int64_t M, int64_t N, int64_t K, GemmPlanInfo *out, int at, int max_out);
int kstream_plan_info(const KItem *items, int n, int64_t N, int aq, const int *item_ids, GemmPlanInfo *out, int at,
                      int max_out);

// Dequantization and the library GEMM (mmq_dequant.hip).  perm: store 4-groups as (0,2,1,3),
// matching act_quant's DEQ form.  blas_gemm returns 0 or a negative code.
hipError_t launch_dequant(int fmt, const uint8_t *A, uint16_t *W, int64_t M, int64_t K, int64_t ldw, bool perm,
                          hipStream_t s);
size_t blas_workspace_bytes();
int blas_gemm(const uint16_t *W, const uint16_t *X, uint16_t *C, int64_t M, int64_t N, int64_t K, int64_t ldc,
              void *ws, size_t ws_bytes, hipStream_t s);

} // namespace gq

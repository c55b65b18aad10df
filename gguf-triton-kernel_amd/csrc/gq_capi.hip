// gq_capi.hip -- the C ABI (include/gguf_mmq.h): argument checks, workspace carving,
// path selection (decode GEMV vs MFMA GEMM) and launches.  Stateless and re-entrant.
#include <climits>
#include <cstdio>
#include <dlfcn.h>
#include <mutex>
#include <cstdarg>
#include <cstdlib>
#include <string>

#include <rccl/rccl.h> // types only: the entry point is resolved at run time (shard_allgather)

#include "../../include/gguf_mmq.h"
#include "gguf_blocks.hpp"
#include "gguf_internal.hpp"

namespace gq {
namespace {

Tuning g_tuning;
std::once_flag g_tuning_once;

bool parse_key(Tuning &t, const char *key, long long v)
{
    auto in = [&](std::initializer_list<long long> ok) {
        for (long long o : ok)
            if (v == o) return true;
        return false;
    };
    const std::string k = key;
    if (k == "GQ_BLAS_MIN_TOKENS") t.blas_min_tokens = v;
    else if (k == "GQ_GEMM_MAX_BYTES") {
        if (v <= 0) return false;
        t.gemm_max_bytes = v < (1LL << 31) ? v : (1LL << 31);
    } else if (k == "GQ_GEMM_I8") t.gemm_i8 = v != 0;
    else if (k == "GQ_NO_FUSED_DECODE") t.fused_decode = v == 0;
    else if (k == "GQ_DECODE_F8_ITC") t.decode_f8_itc = v != 0;
    else if (k == "GQ_SGEMM_STREAMK") t.sgemm_streamk = v < 0 ? -1 : (v != 0);
    else if (k == "GQ_DECODE_Q6_IMG") {
        if (!in({-1, 0, 1})) return false;
        t.decode_q6_img = (int)v;
    }
    else if (k == "GQ_GEMM_AQ") t.gemm_aq = v != 0;
    else if (k == "GQ_GEMM_RG") {
        if (!in({0, 1, 2})) return false;
        t.gemm_rg = (int)v;
    } else if (k == "GQ_GEMM_SPLITS") {
        if (v < 0) return false;
        t.gemm_splits = v;
    } else if (k == "GQ_GEMM_PARTIAL") t.gemm_partial_f32 = v != 0; // 1 = f32
    else if (k == "GQ_SKINNY") {
        if (!in({-1, 0, 1})) return false;
        t.skinny = (int)v;
    } else if (k == "GQ_SKINNY_RG") {
        if (!in({0, 1, 2, 3, 4})) return false;
        t.skinny_rg = (int)v;
    } else if (k == "GQ_RGEMM") {
        if (!in({-1, 0, 1})) return false;
        t.rgemm = (int)v;
    } else if (k == "GQ_SGEMM") {
        if (!in({-1, 0, 1})) return false;
        t.sgemm = (int)v;
    } else if (k == "GQ_SGEMM_SPLITS") {
        if (v < 0 || v > 4096) return false;
        t.sgemm_splits = (int)v;
    } else if (k == "GQ_RGEMM_ILC") t.rgemm_ilc = v != 0;
    else if (k == "GQ_RGEMM_ESTORE") {
        if (!in({-1, 0, 1})) return false;
        t.rgemm_estore = (int)v;
    } else if (k == "GQ_SGEMM_FULL") {
        t.sgemm_full = v < 0 ? -1 : (v != 0);
    } else if (k == "GQ_CUS") {
        if (v < 0 || v > 1024) return false;
        t.cus = (int)v;
    } else if (k == "GQ_KSTREAM") {
        if (!in({-1, 0, 1})) return false;
        t.kstream = (int)v;
    } else if (k == "GQ_ABLATE") t.ablate = (int)v;
    else return false;
    return true;
}

void tuning_from_env(Tuning &t)
{
    t = Tuning{};
    static const char *const keys[] = {"GQ_BLAS_MIN_TOKENS", "GQ_GEMM_MAX_BYTES", "GQ_GEMM_I8", "GQ_NO_FUSED_DECODE",
                                       "GQ_DECODE_Q6_IMG", "GQ_DECODE_F8_ITC", "GQ_GEMM_AQ", "GQ_GEMM_RG", "GQ_GEMM_SPLITS",
                                       "GQ_GEMM_PARTIAL", "GQ_SKINNY", "GQ_SKINNY_RG", "GQ_RGEMM", "GQ_SGEMM",
                                       "GQ_SGEMM_SPLITS", "GQ_SGEMM_STREAMK", "GQ_RGEMM_ILC", "GQ_RGEMM_ESTORE", "GQ_SGEMM_FULL", "GQ_CUS",
                                       "GQ_KSTREAM", "GQ_ABLATE"};
    for (const char *k : keys) {
        const char *e = getenv(k); // the only getenv of the library: once per process
        if (!e || !*e) continue;
        long long v;
        if (std::string(k) == "GQ_GEMM_PARTIAL") v = std::string(e) == "f32";
        else v = atoll(e);
        if (!parse_key(t, k, v)) fprintf(stderr, "gguf_mmq: ignoring %s=%s (out of range)\n", k, e);
    }
}

} // namespace

const Tuning &tuning()
{
    std::call_once(g_tuning_once, [] { tuning_from_env(g_tuning); });
    return g_tuning;
}

int set_tuning(const char *key, long long value)
{
    tuning();
    Tuning t = g_tuning;
    if (!key || !parse_key(t, key, value)) return -1;
    g_tuning = t;
    return 0;
}

void reset_tuning()
{
    tuning();
    Tuning t;
    tuning_from_env(t); // built aside and published by one assignment, as set_tuning does
    g_tuning = t;
}

int num_cus()
{
    if (tuning().cus > 0) return tuning().cus; // test override (GQ_CUS)
    static int cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cached[dev] <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev] = n;
    }
    return cached[dev];
}

// ---- the planner: host-only; everything the ABI decides about a call is decided here, once ----
namespace {

// One row per gq_type of what is the ABI's own: the type's names and the kind of its device
// quantizer (launch_quant_blocks; -1: none, gq_quantize_<lname> on the host).  The block geometry
// and whether the streaming GEMM is the type's only GEMM kernel (q8_1_only) are gguf_blocks.hpp's kFmt.
struct TypeInfo {
    const char *name, *lname;
    int quant_kind;
};
constexpr TypeInfo kTypes[] = {{"Q8_0", "q8_0", 0},  {"Q4_K", "q4_k", 1},  {"Q6_K", "q6_k", 2},
                               {"Q5_K", "q5_k", -1}, {"Q3_K", "q3_k", -1}, {"Q2_K", "q2_k", -1},
                               {"Q4_0", "q4_0", 4}};
static_assert(GQ_Q8_0 == 0 && GQ_Q4_K == 1 && GQ_Q6_K == 2 && GQ_Q5_K == 3 && GQ_Q3_K == 4 && GQ_Q2_K == 5 && GQ_Q4_0 == 6 &&
                  sizeof(kTypes) / sizeof(kTypes[0]) == kNumFmts,
              "kTypes and kFmt are indexed by gq_type");
bool known_type(int t) { return known_fmt(t); }
// (an unknown type answers with Q6_K's row, as gq_block_bytes always did: callers detect a type by it;
// fmt_info does the same for the block)
const TypeInfo &type_info(int t) { return kTypes[known_type(t) ? t : (int)GQ_Q6_K]; }

size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// Decode path up to this many tokens; beyond it the fp16-MFMA GEMM.
constexpr int64_t kGemvMaxTokens = 4; // 5..8 tokens: the MFMA GEMM (15.9 us at 16 tokens vs 22.3 us decode at 8, Q4_K 4096^2)

// (K % 128 != 0 is only possible for Q8_0 and Q4_0, so the choice depends on N and K alone and
// gq_act_prepare, which does not know the weight type, makes the same one.)
bool use_gemv(int64_t N, int64_t K) { return N <= kGemvMaxTokens || !gemm_supported(Q8_0, K); }

// Library-GEMM path (dequantize W to fp16 + hipBLASLt) from this many tokens on; the
// override GQ_BLAS_MIN_TOKENS (0 = never) is for tuning and tests.
// default 768: measured crossover (11008x4096 Q4_K 512 tokens 90 vs 121 us, 4096^2 1024 tokens)
bool use_blas(int64_t N, int64_t K, const Tuning &u)
{
    return !use_gemv(N, K) && u.blas_min_tokens > 0 && N >= (int64_t)u.blas_min_tokens;
}

// The MFMA GEMM addresses its operands with 32-bit buffer offsets: one launch covers at most
// this many weight bytes and this many activation bytes; larger calls are cut into row / token
// chunks (launched back to back on the stream, reusing the workspace).
// (GQ_GEMM_MAX_BYTES lowers the limit: tests cut small calls into many chunks.)
int64_t gemm_max_bytes(const Tuning &u)
{
    const int64_t lim = (int64_t)1 << 31;
    return u.gemm_max_bytes > 0 && u.gemm_max_bytes < lim ? (int64_t)u.gemm_max_bytes : lim;
}
int64_t gemm_rows_per_launch(int t, int64_t M, int64_t K, const Tuning &u)
{
    const int64_t r = gemm_max_bytes(u) / row_bytes(t, K) / 256 * 256; // whole 256-row tiles
    return r < 256 ? 256 : (r < M ? r : M);
}
int64_t gemm_toks_per_launch(int64_t N, int64_t K, const Tuning &u)
{
    const int64_t n = gemm_max_bytes(u) / (2 * K) / 128 * 128; // whole 128-token tiles
    return n < 16 ? 16 : (n < N ? n : N);
}

// Q8_0 on the MFMA GEMM path: int8 activations x int8 weights (v_mfma_i32_16x16x32_i8 + per-block
// fp32 scaling) instead of fp16 x~ x dequantized weights.  GQ_GEMM_I8=0/1 overrides.
bool use_i8(int t, int64_t N, int64_t K, const Tuning &u)
{
    return t == GQ_Q8_0 && !use_gemv(N, K) && !use_blas(N, K, u) && u.gemm_i8 != 0;
}

constexpr int64_t kRgemmMinTokens = 5, kRgemmMultiRoundTokens = 32, kRgemmMultiRoundTokensQ4 = 64;
// Skinny-token kernel (mmq_skinny.hip).  By type and token count only (a row subset runs the
// same arithmetic as the whole matrix): by default Q4_K and Q8_0 at 5..16 tokens, where it
// measured faster than the LDS-DMA GEMM (profiles/r03/tails/route_sw.log, step incl. act_quant,
// 16 tokens: Q4_K 4096^2 9.7 vs 12.0 us, 11008x4096 15.3 vs 22.2, 4096x11008 16.5 vs 19.6; Q8_0
// 4096^2 11.3 vs 13.1, 11008x4096 19.4 vs 24.3).  Q6_K stays on the GEMM: faster on 4096-row
// matrices (11.6 vs 13.0) but 28672x8192 72 vs 95, and the choice may not depend on M; 17..32
// tokens: mixed (Q4_K +8% / -5% by shape), the GEMM.  GQ_SKINNY=1: every type at 1..32 tokens
// the GEMM path would take (tests), 0: off.
constexpr int64_t kSkinnyMinTokens = 5, kSkinnyMaxTokens = 16, kSkinnyForcedMax = 32;
bool use_skinny(int t, int form, int64_t N, int act, const Tuning &u)
{
    if (form != AF_F16 || u.skinny == 0 || q8_1_only(t)) return false;
    if (u.skinny == 1) return N <= kSkinnyForcedMax;
    // the fp8 variant has no decode kernel: its 1..4 tokens take the skinny kernel too
    const int64_t lo = act == GQ_ACT_FP8_E4M3 ? 1 : kSkinnyMinTokens;
    return (t == GQ_Q4_K || t == GQ_Q8_0) && N >= lo && N <= kSkinnyMaxTokens;
}

// A knob of the LDS-DMA GEMM set (tests, A/B of those kernels): the automatic
// resident / streaming routes stand aside so the call reaches the kernel the knob is for.
bool gemm_knob_pinned(const Tuning &u) { return u.gemm_splits > 0 || u.gemm_rg || u.gemm_partial_f32; }

// Resident-split GEMM (mmq_rgemm.hip: 256 rows x <= 128 tokens x one super-block per workgroup,
// the split's operands loaded once; profiles/r04/).  By default where its grid is one round of
// the chip and at least half of it (a 4096-row matrix at K = 4096: 16 x 16 workgroups) and the
// call needs no 2 GiB chunking; the q8_1 activations are quantized inside it (gq_mmq_ex) or read
// prepared (gq_mmq_prepared).  With split-K over every super-block its partial sums differ from
// gemm_kernel's (other splits), so a forced split factor (GQ_GEMM_SPLITS) keeps gemm_kernel.
// GQ_RGEMM=1: wherever it applies (tests), 0: off.  p: its plan.
bool use_rgemm(int t, int form, int64_t M, int64_t N, int64_t K, const Tuning &u, RGemmPlan &p)
{
    const int rg = u.rgemm;
    if (q8_1_only(t)) return false; // (no resident form: the streaming GEMM, whatever GQ_RGEMM says)
    if (rg == 0 || form != AF_F16 || use_gemv(N, K) || use_blas(N, K, u) || K % 256 != 0) return false;
    if (gemm_rows_per_launch(t, M, K, u) < M || gemm_toks_per_launch(N, K, u) < N) return false;
    p = plan_rgemm(M, N, K);
    if (!p.ok) return false;
    if (rg == 1) return true;
    if (gemm_knob_pinned(u) || N < kRgemmMinTokens) return false;
    // one round of the chip at the workgroups a CU holds (Q4_K at 16 tokens: three -- 11008x4096
    // and 4096x11008 at 688 workgroups); up to 32 tokens, up to four rounds (the one-super-block
    // workgroups are short, so later rounds fill in behind the first; step us, default route ->
    // resident, profiles/r04/b6_rg2.txt: Q4_K 22016x4096 x16 27.4 -> 21.6, x8 26.5 -> 20.9,
    // 14336x4096 x16 18.3 -> 14.5, 4096x14336 x16 20.6 -> 14.6, 11008x4096 x32 22.3 -> 15.6;
    // Q6_K 11008x4096 x16 22.2 -> 21.0; Q8_0 11008x4096 x16 20.1 -> 19.4)
    const int64_t grid = (int64_t)p.tiles_m * p.tiles_n * p.splits, cus = num_cus();
    // (Q4_K to 64 tokens: 11008x4096 x48/x64 25.3/25.4 -> 19.5/20.5, 22016x4096 x64 40.6 -> 36.6,
    // 4096x11008 x64 23.1 -> 18.7; not at 128, nor Q6_K at 64: profiles/r04/b7_rg64.txt)
    const int64_t rounds = N <= (t == GQ_Q4_K ? kRgemmMultiRoundTokensQ4 : kRgemmMultiRoundTokens) ? 4 : 1;
    return grid <= rounds * cus * rgemm_per_cu(t, p.nb) && 2 * grid >= cus;
}

// K-chunked streaming MMQ (mmq_kstream.hip): 5..32 tokens (the fp8 variant from 3: its decode
// form covers 1..2), K % 256 == 0, M % 16 == 0; one launch for K <= 4096 (x~ quantized in-kernel
// from the raw activations, or read prepared).  GQ_KSTREAM=1: wherever it applies, 0: off.
// By default on the prepared calls (x~ read as act_quant wrote it; single and grouped) and the
// raw grouped launch: 5..32 tokens measured 7-12% under the routes before it (MMQ us, default -> kstream, round 5
// profiles/r05/ks_ab.txt: Q4_K 4096^2 x16 9.25 -> 7.96, 11008x4096 x16 15.31 -> 13.65,
// 22016x4096 x16 24.23 -> 22.12, x32 30.52 -> 27.72, x8 24.02 -> 21.69; Q6_K 4096^2 x16 10.55 ->
// 9.32; Q8_0 11008x4096 x16 18.05 -> 16.90).  Quantizing in-kernel (gq_mmq_ex) it is slower on the
// small matrices (every workgroup quantizes its whole K of x): a raw call takes it on the tall ones.
// A K longer than 4096 is cut into ranges summed by a second launch (fp32 partials in the
// workspace): by default only inside a grouped launch (the layer's ffn_down beside the K = 4096
// projections); split = false asks for the one-launch form.
bool use_kstream(int t, int form, int64_t M, int64_t N, int64_t K, int act, bool prepared, bool split, const Tuning &u)
{
    const int ks = u.kstream;
    if (ks == 0 || form != AF_F16 || use_blas(N, K, u) || !kstream_ok(t, M, N, K)) return false;
    // (q8_1 at 3..4 tokens: the grouped decode -- the prepared workspace holds the decode's SOA
    // q8_1 form there, not the fp16 x~ the stream reads; profiles/r06/kstream_nmin3_ab.txt)
    if (N < (act == GQ_ACT_FP8_E4M3 ? 3 : 5)) return false;
    if (kstream_splits(K) > 1 && !split && ks != 1) return false;
    if (ks == 1) return true;
    if (gemm_knob_pinned(u)) return false; // (as the resident / streaming routes: the pinned GEMM takes the call)
    if (prepared) return true;
    // a raw call quantizes in-kernel (every workgroup its whole K of x): ahead of the resident GEMM
    // on the tall matrices at 5..16 tokens (Q4_K 11008 / 14336 / 22016 x4096 x16 15.79 / 17.74 /
    // 25.14 -> 15.41 / 17.36 / 23.23 us, Q6_K 11008 19.79 -> 19.15, Q8_0 11008 18.69 -> 18.33, x8
    // 15.61 -> 15.37), behind it on 4096-row matrices (9.27 -> 11.18) and at 32 tokens (18.51 ->
    // 23.98) -- profiles/r05/raw_kstream_ab.txt
    return act == GQ_ACT_Q8_1 && N <= 16 && M >= 8192;
}
// its 32-bit buffer offsets over the activations (rows ldx apart) and the output (rows ldc apart),
// and its 8-byte buffer stores of four outputs at C + tok*ldc + row (row % 4 == 0): aligned only
// with ldc % 4 == 0 and C on an 8-byte boundary (c_aligned; c8()).  Every other C takes the call's
// next route, whose epilogues are plain global stores.
bool c8(const void *C) { return ((uintptr_t)C & 7) == 0; }
bool kstream_fits(int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldc, bool c_aligned)
{
    return ((N - 1) * ldx + K) * 2 < ((int64_t)1 << 31) && ((N - 1) * ldc + M) * 4 < ((int64_t)1 << 31) && ldc % 4 == 0 &&
           c_aligned;
}
// An item of a grouped launch (gq_mmq_grouped_ex, gq_mmq_grouped_prepared): the stream wherever
// it applies (the prepared rule; split: K ranges allowed)
bool grouped_kstream_item(int t, int act, int64_t M, int64_t N, int64_t K, int64_t ldx, int64_t ldc, const void *C,
                          bool split, const Tuning &u)
{
    return use_kstream(t, AF_F16, M, N, K, act, true, split, u) && kstream_fits(M, N, K, ldx, ldc, c8(C));
}

// Streaming 256-row GEMM (mmq_rgemm.hip sgemm_kernel) on the prepared x~, where the resident
// form does not apply (its grid is more than one round of the chip, or under half of one): by
// default from 17 tokens for every type, and Q6_K from 5 (the skinny kernel keeps Q4_K / Q8_0
// at 5..16) -- profiles/r04/sg_v1.txt, sg_n.txt, sg_small.txt (MMQ us, old route -> sgemm): Q6_K
// 28672x8192 x32/x64/x128/x256/x512 73.2/79.9/110.1/207.8/386.5 -> 71.5/78.1/102.2/178.4/342.3,
// 8192x28672 x64/x128 81.1/107.0 -> 75.5/96.5; Q8_0 11008x4096 x64/x128/x256 27.2/36.5/54.9 ->
// 23.8/28.8/45.4; Q4_K 11008x4096 x32/x64/x128 20.8/24.4/30.7 -> 20.0/22.7/28.9 (x256 46.8 vs
// 47.3); Q6_K 11008x4096 x16 23.5 -> 19.8.  GQ_SGEMM=1: wherever it applies (tests, A/B), 0: off.
constexpr int64_t kSgemmMinTokens = 17, kSgemmQ6MinTokens = 5;
bool use_sgemm(int t, int form, int64_t M, int64_t N, int64_t K, const Tuning &u)
{
    if (form != AF_F16 || use_gemv(N, K) || use_blas(N, K, u) || K % 256 != 0) return false;
    // Q5_K's, Q3_K's, Q2_K's and Q4_0's only GEMM kernel: every 5..BLAS-threshold token count, whatever GQ_SGEMM or a pinned
    // knob of the other GEMMs says; rows over the per-launch limit are cut into chunks
    if (q8_1_only(t)) {
        // the call's tokens go into every launch (rows alone are cut).  Counted as the other GEMMs
        // count them, in whole 128-token tiles of x~ -- but for a type whose 768 rows weigh less than
        // 128 tokens' x~ at every K (768 * block bytes < 128 * 2 * block elements: Q2_K alone, 252 K
        // against 256 K bytes) that count admits 16 tokens under any limit that cuts its rows at
        // all, so for it the x~ bytes are counted exactly
        const FmtInfo &ti = fmt_info(t);
        const bool toks_fit = 768 * ti.bytes < 256 * ti.qk ? N * 2 * K <= gemm_max_bytes(u)
                                                              : gemm_toks_per_launch(N, K, u) >= N;
        return M > 0 && toks_fit && 256 * row_bytes(t, K) < ((int64_t)1 << 31);
    }
    if (u.sgemm == 0) return false;
    if (gemm_rows_per_launch(t, M, K, u) < M || gemm_toks_per_launch(N, K, u) < N) return false;
    if (!plan_sgemm(M, N, K, u.sgemm_splits).ok) return false;
    if (u.sgemm == 1) return true;
    if (gemm_knob_pinned(u)) return false;
    return N >= kSgemmMinTokens || (t == GQ_Q6_K && N >= kSgemmQ6MinTokens);
}
// The streaming GEMM of one matrix as the grouped kernel's one-part stream-K plan (GQ_SGEMM_STREAMK=1,
// splits not pinned, tiles within one round of the chip): every workgroup L or L+1 super-blocks
// instead of whole-tile splits (Q6_K 28672x8192 x128: 224 workgroups x 16 super-blocks -> 256 x
// 14).  Measured no faster (104.7 vs 101.9 us there; 11008x4096 x128 33.7 vs 28.9: a workgroup
// of 2-3 super-blocks spanning two tiles fills and drains its ring twice and stores two
// partials; profiles/r04/b4_sk.txt), so off by default.
bool sgemm_streamk(int t, int64_t M, int64_t N, int64_t K, const Tuning &u, SGroupItem &it, SGroupPlan &g)
{
    if (u.sgemm_splits > 0 || u.sgemm_streamk <= 0) return false;
    it = SGroupItem{t, nullptr, nullptr, nullptr, M, M, K};
    g = plan_sgemm_grouped(&it, 1, N, 0);
    return g.ok && g.streamk;
}
size_t sgemm_partial_bytes(int t, int64_t M, int64_t N, int64_t K, const Tuning &u)
{
    SGroupItem it;
    SGroupPlan g;
    return sgemm_streamk(t, M, N, K, u, it, g) ? g.partial_bytes : plan_sgemm(M, N, K, u.sgemm_splits).partial_bytes;
}

// Decode token counts (q8_1: the GEMV tokens, fp8: 1-2): gq_act_prepare also keeps an fp16 copy
// of the activations at the end of the activation part, so that gq_mmq_prepared runs the same
// one-launch decode as gq_mmq (bit-identical to it) instead of the GEMV on the SOA form (Q6_K
// 28672x8192 x1 60.6 -> 35.4 us; profiles/r05/prepared_decode_ab.txt)
// The copy only where a weight type's fused decode can run at (N, K) (gq_act_prepare does not
// know the type; e.g. 4 tokens at K = 11008 fit no type's LDS image: no copy, the GEMV)
bool prep_raw(int act, int64_t N, int64_t K)
{
    const bool fp8 = act == GQ_ACT_FP8_E4M3;
    if (fp8 ? !(N <= 2 && gemm_supported(Q8_0, K)) : !use_gemv(N, K)) return false;
    for (int t : {GQ_Q8_0, GQ_Q4_K, GQ_Q6_K})
        if ((t == GQ_Q8_0 || K % 256 == 0) && decode_fused_ok(t, N, K, fp8)) return true;
    return false;
}

// The workspace: the activation part (what gq_act_prepare[_ex] writes; depends on act, N, K only),
// then the partials.  Decode token counts: SOA q8_1 codes + d + s; the GEMM paths: fp16 x~ [N][K],
// then codes [N][K] and block-major scales d, s [K/32][scale_ld(N)] (s: the integer skinny
// kernel); the fp8 variant: x~ alone.  Every piece 256-byte aligned.
int64_t scale_ld(int64_t N) { return (N + 3) & ~(int64_t)3; }
struct Carved {
    int8_t *xq;       // SOA codes (decode) / GEMM codes (int8 form)
    float *xd, *xs;   // SOA d, s (decode) / GEMM block-major scales
    uint16_t *xdeq;
    uint16_t *xraw;   // decode token counts: the fp16 activations (rows K apart; prep_raw)
    float *partials;
    size_t act_bytes; // the activation part
};
Carved carve(int act, void *workspace, int64_t N, int64_t K)
{
    uintptr_t at = (uintptr_t)workspace;
    auto take = [&at](size_t bytes) {
        const uintptr_t p = at;
        at += align_up(bytes);
        return p;
    };
    const size_t nk = (size_t)N * K, soa = (size_t)N * (K / 32) * sizeof(float), sc = (size_t)(K / 32) * scale_ld(N) * 4;
    Carved c{};
    if (act == GQ_ACT_FP8_E4M3) {
        c.xdeq = (uint16_t *)take(nk * 2);
    } else if (use_gemv(N, K)) {
        c.xq = (int8_t *)take(nk), c.xd = (float *)take(soa), c.xs = (float *)take(soa);
    } else {
        c.xdeq = (uint16_t *)take(nk * 2), c.xq = (int8_t *)take(nk), c.xd = (float *)take(sc), c.xs = (float *)take(sc);
    }
    if (prep_raw(act, N, K)) c.xraw = (uint16_t *)take(nk * 2);
    c.partials = (float *)at;
    c.act_bytes = at - (uintptr_t)workspace;
    return c;
}
size_t act_bytes(int act, int64_t N, int64_t K) { return carve(act, nullptr, N, K).act_bytes; }

// One call as the planner sees it.  A raw call (gq_mmq_ex) is routed by the strides and the
// alignment of its activations too; a shape-only query (the workspace sizes, gq_debug_route)
// assumes what shape_call() fills in: contiguous rows, B 16-byte aligned, C 8-byte aligned.
struct Call {
    int t, act;
    int64_t M, N, K;
    bool prepared;   // gq_mmq_prepared: x~ is in the workspace as gq_act_prepare wrote it
    int64_t ldb, ldc;
    bool b_aligned;  // raw: 16-byte rows (ldb % 8 == 0, B & 15 == 0), what the in-kernel quantizers load
    bool c_aligned;  // C & 7 == 0 (kstream_fits)
};
Call shape_call(int t, int act, int64_t M, int64_t N, int64_t K, bool prepared)
{
    return Call{t, act, M, N, K, prepared, K, M, true, true};
}

// The kernel family (gq_debug_route: route_name()).  K_NONE: nothing to run (M or N zero) or no
// kernel for the shape (GQ_EUNSUPPORTED); K_SGEMM_STREAMK: the streaming GEMM as the grouped
// kernel's one-part stream-K plan; K_GEMM: the LDS-DMA GEMM.  Skinny, sgemm and gemm run per chunk.
enum Kernel { K_NONE, K_DECODE, K_GEMV, K_BLAS, K_KSTREAM, K_RGEMM, K_SKINNY, K_SGEMM, K_SGEMM_STREAMK, K_GEMM };

// Everything the ABI needs to know about one call.
// The q8_1 activations (the reference's semantics) go to the fused decode / GEMV (N <= 4), the
// MFMA GEMMs or, from GQ_BLAS_MIN_TOKENS, dequant + hipBLASLt; the fp8 variant (GQ_ACT_FP8_E4M3)
// is quantized to e4m3 codes and widened to fp16 x~ by act_quant (ACT_F8DEQ), then runs every
// fp16-activation kernel as q8_1's x~ does (skinny from one token: there is no fp8 GEMV).
// (Widening the codes inside the GEMM instead, the round-2 AF_F8 form, cost 12-55% over the q8_1
// path: profiles/r03/s3/fp8_deq_route.log.)
struct Plan {
    Kernel kernel = K_NONE;
    // raw: one launch on the caller's fp16 activations, quantized inside the kernel (aq: 1 as q8_1,
    // 2 as the fp8 variant), bit-identical to the act_quant form it would read.  A raw call whose
    // plan is not raw is act_quant (prepare(): forms) + the PREPARED call's plan, which may name
    // another kernel (by default the K-chunked stream takes every prepared 5..32-token call, a raw
    // one only on tall matrices); gq_debug_route(prepared = 0) names this plan's.
    bool raw = false;
    int aq = 0;
    int form = AF_F16, forms = 1; // the GEMM's activation form; the act_quant forms prepare() writes for it
    int64_t rows = 0, toks = 0;   // rows / tokens per launch of the chunked kernels
    RGemmPlan rg;                 // K_RGEMM; K_SGEMM: the whole matrix's (a row chunk plans its own)
    SGroupItem item{};            // K_SGEMM_STREAMK
    SGroupPlan sg;
    GemmPlan gemm;                // raw K_GEMM
    size_t act_bytes = 0, partial_bytes = 0;
    size_t ws_bytes() const { return act_bytes + partial_bytes; } // the workspace this call needs
};

Plan plan_call(const Call &c, const Tuning &u)
{
    const int t = c.t, act = c.act;
    const int64_t M = c.M, N = c.N, K = c.K;
    const bool fp8 = act == GQ_ACT_FP8_E4M3, work = M > 0 && N > 0;
    Plan p;
    const bool gemv = !fp8 && use_gemv(N, K), blas = use_blas(N, K, u);
    p.form = !fp8 && use_i8(t, N, K, u) ? AF_I8 : AF_F16;
    p.forms = p.form == AF_I8 ? 2 : 1;
    // the one-launch decode; the fp8 variant's own form (mmq_decode.hip FP8: fp16 dot products,
    // 3-4x the int8 form's VALU) at 1-2 tokens: at 3-4 the skinny kernel / GEMM is faster (7B layer
    // x4 83 vs 73 us; profiles/r03/s3/fp8_decode.log)
    const bool fused = u.fused_decode && (fp8 ? N <= 2 : gemv) && decode_fused_ok(t, N, K, fp8);
    if (fused && !c.prepared) { // on the caller's activations: no workspace at all
        p.kernel = K_DECODE;
        p.raw = true;
        return p;
    }
    p.act_bytes = act_bytes(act, N, K);

    // the GEMM token counts: every rule once
    const bool gemm_tokens = work && !blas && !gemv && gemm_supported(t, K);
    bool skinny = false, rgemm = false, sgemm = false, kstream = false, streamk = false;
    RGemmPlan rg, sg;
    if (gemm_tokens) {
        skinny = use_skinny(t, p.form, N, act, u);
        // (<= 32 skinny tokens are never cut: their x~ is far below the guard, and the token
        // count sets the kernel's K split)
        p.rows = gemm_rows_per_launch(t, M, K, u);
        p.toks = skinny ? N : gemm_toks_per_launch(N, K, u);
        rgemm = use_rgemm(t, p.form, M, N, K, u, rg);
        sgemm = use_sgemm(t, p.form, M, N, K, u);
        kstream = use_kstream(t, p.form, M, N, K, act, c.prepared, false, u) &&
                  kstream_fits(M, N, K, c.prepared ? K : c.ldb, c.ldc, c.c_aligned);
        if (sgemm) {
            streamk = p.rows >= M && sgemm_streamk(t, M, N, K, u, p.item, p.sg);
            sg = plan_sgemm(M, N, K, u.sgemm_splits);
        }
    }
    // the kernels quantizing 16-byte rows themselves: a prepared call reads x~ instead
    const bool raw_ok = !c.prepared && c.b_aligned, x_ok = c.prepared || raw_ok;

    if (!work || (!blas && !gemv && !gemm_tokens)) { // (or the fp8 variant at a K the launch refuses: sized only)
    } else if (fused && prep_raw(act, N, K)) {
        p.kernel = K_DECODE; // gq_mmq's one-launch decode on the prepared copy
    } else if (blas || gemv) {
        p.kernel = blas ? K_BLAS : K_GEMV;
    } else if (kstream && x_ok) {
        p.kernel = K_KSTREAM;
        p.raw = raw_ok;
    } else if (rgemm && (u.skinny != 1 || !skinny) && x_ok) {
        // The resident GEMM where it applies, ahead of the skinny kernel (4096^2 x16 step: Q4_K 6.8 vs
        // 9.7 us, Q8_0 7.8 vs 11.2, Q6_K 8.1 vs 12.9; x8 Q4_K 6.8 vs 9.3 -- profiles/r04/rg_small.txt)
        // unless the skinny kernel is forced (GQ_SKINNY=1)
        p.kernel = K_RGEMM;
        p.rg = rg;
        p.raw = raw_ok;
    } else if (skinny) {
        p.kernel = K_SKINNY;
    } else if (sgemm) {
        p.kernel = streamk ? K_SGEMM_STREAMK : K_SGEMM;
        if (!streamk) p.rg = sg;
    } else if (!q8_1_only(t)) { // (Q5_K / Q3_K / Q2_K / Q4_0: the streaming GEMM or nothing, GQ_EUNSUPPORTED)
        p.kernel = K_GEMM;
        if (!c.prepared && act == GQ_ACT_Q8_1 && p.form == AF_F16 && p.rows >= M && p.toks >= N) {
            // 16/32-token tiles whose split fits LDS: the GEMM quantizes the activations itself (no
            // act_quant launch; bit-identical to the DEQ form it would read; any fp16-aligned rows)
            p.gemm = plan_gemm(t, M, N, K, p.form);
            p.raw = gemm_aq_ok(p.gemm);
            p.gemm.aq = p.raw;
        }
    }
    p.aq = p.raw ? (fp8 ? 2 : 1) : 0;

    // The workspace after the activations: fp16 W + hipBLASLt's own, or split-K partials -- the
    // largest need over the routes this shape can reach, not the chosen kernel's alone: the size
    // may not depend on strides or alignment (a raw call that cannot take its one-launch kernel is
    // act_quant + the prepared call), every chunk shape of a cut call counts, and a forced K-chunked
    // stream has its K ranges.  ABI-visible (gguf_mmq.h bumps gq_version when a size grows).
    if (blas) {
        p.partial_bytes = align_up((size_t)M * K * 2) + blas_workspace_bytes();
    } else if (gemm_tokens && q8_1_only(t)) {
        // the streaming GEMM per chunk of p.rows rows (rows are independent): the largest chunk shape's
        size_t b = 0;
        for (int64_t mc : {p.rows, M % p.rows})
            if (sgemm && mc > 0) b = std::max(b, sgemm_partial_bytes(t, mc, N, K, u));
        p.partial_bytes = align_up(b);
    } else if (gemm_tokens) {
        size_t b = rgemm ? rg.partial_bytes : sgemm ? (streamk ? p.sg.partial_bytes : sg.partial_bytes) : 0;
        if (u.kstream == 1 && kstream_ok(t, M, N, K) && N <= 32) { // (its K ranges)
            const KItem it{t, nullptr, nullptr, K, nullptr, M, M, K};
            b = std::max(b, kstream_partial_bytes(&it, 1, N));
        }
        // the LDS-DMA GEMM over the launch shapes (full and remainder chunks; the kernel is chosen
        // by the call's token count, so every chunk runs the same arithmetic)
        for (int64_t mc : {p.rows, M % p.rows})
            for (int64_t nc : {p.toks, N % p.toks})
                if (!skinny && mc > 0 && nc > 0) b = std::max(b, plan_gemm(t, mc, nc, K, p.form).partial_bytes);
        p.partial_bytes = align_up(b);
    }
    return p;
}

// gq_debug_route's text for a plan
const char *route_name(const Call &c, const Plan &p)
{
    switch (p.kernel) {
    case K_DECODE: return "stream_decode_kernel";
    case K_BLAS: return "dequant_kernel + hipBLASLt";
    case K_GEMV: return "gemv_kernel";
    case K_KSTREAM: return kstream_splits(c.K) > 1 ? "kstream_kernel + kstream_reduce_kernel" : "kstream_kernel";
    case K_RGEMM:
        return p.rg.splits == 1        ? "rgemm_kernel"
               : rgemm_ilc(c.t, p.rg) ? "rgemm_kernel (in-launch split-K sum)"
                                      : "rgemm_kernel + gemm_reduce_f16_kernel";
    case K_SKINNY: return "skinny_kernel";
    case K_SGEMM_STREAMK: return "sgemm_grouped_kernel + reduce_grouped_kernel (stream-K)";
    case K_SGEMM:
        return p.rg.splits == 1 ? "sgemm_kernel"
               : sgemm_ilc(p.rg) ? "sgemm_kernel (in-launch split-K sum)"
                                 : "sgemm_kernel + gemm_reduce_f16_kernel";
    case K_GEMM: return "gemm_kernel + gemm_reduce_f16_kernel";
    case K_NONE: break; // (Q5_K / Q3_K / Q2_K never reach the LDS-DMA GEMM: GQ_EUNSUPPORTED)
    }
    return "none";
}

} // namespace
} // namespace gq

namespace {

thread_local std::string g_err;

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// GQ_OK, or GQ_EHIP with the launch named in the text
int hip_rc(hipError_t e, const char *what = nullptr)
{
    if (e == hipSuccess) return GQ_OK;
    if (!what) return fail(GQ_EHIP, "HIP launch failed: %s", hipGetErrorString(e));
    return fail(GQ_EHIP, "HIP launch failed (%s): %s", what, hipGetErrorString(e));
}

// ---- row sharding (gq_mmq_sharded) ----
constexpr int64_t kShardAlign = 64; // dist/row_shard.py shard_rows(align=64)

void shard_geom(int64_t M, int world, int rank, int64_t &row0, int64_t &rows, int64_t &R)
{
    R = (M + world - 1) / world;
    R = (R + kShardAlign - 1) / kShardAlign * kShardAlign;
    row0 = (int64_t)rank * R < M ? (int64_t)rank * R : M;
    const int64_t end = row0 + R < M ? row0 + R : M;
    rows = end - row0;
}

// C[n][m] = G[m / R][n][m % R]; VEC = 8: 8 columns (16 bytes) per thread (R % 8 == 0, so a
// group never straddles two shards; used when C's rows and M allow 16-byte stores)
template <int VEC>
__global__ __launch_bounds__(256) void assemble_kernel(const uint16_t *__restrict__ G, uint16_t *__restrict__ C,
                                                       int64_t N, int64_t R, int64_t M, int64_t ldc)
{
    const int64_t groups = (M + VEC - 1) / VEC;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N * groups;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t n = i / groups, m = (i - n * groups) * VEC;
        const int64_t g = m / R, r = m - g * R;
        const uint16_t *src = G + (g * N + n) * R + r;
        uint16_t *dst = C + n * ldc + m;
        if constexpr (VEC == 8) {
            *(uint4 *)dst = *(const uint4 *)src;
        } else {
            *dst = *src;
        }
    }
}

hipError_t launch_assemble(const uint16_t *G, uint16_t *C, int64_t N, int64_t R, int64_t M, int64_t ldc,
                           hipStream_t s)
{
    const bool vec = M % 8 == 0 && ldc % 8 == 0 && ((uintptr_t)C & 15) == 0 && ((uintptr_t)G & 15) == 0;
    const int64_t items = N * (vec ? M / 8 : M);
    const int64_t blocks = (items + 255) / 256 < 4096 ? (items + 255) / 256 : 4096;
    if (vec) assemble_kernel<8><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(G, C, N, R, M, ldc);
    else assemble_kernel<1><<<dim3((unsigned)blocks), dim3(256), 0, s>>>(G, C, N, R, M, ldc);
    return hipGetLastError();
}

// RCCL's all-gather, looked up in the process (the caller's RCCL, whose communicator we are
// handed); librccl.so.1 is opened by soname only if nothing in the process exports it
using AllGatherFn = decltype(&ncclAllGather);
AllGatherFn shard_allgather()
{
    static AllGatherFn fn = nullptr;
    static std::once_flag once;
    std::call_once(once, [] {
        void *sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
        if (!sym) {
            if (void *h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL)) sym = dlsym(h, "ncclAllGather");
        }
        fn = (AllGatherFn)sym;
    });
    return fn;
}

// every rank's need: the local MMQ's workspace is not monotone in the row count (fewer rows ->
// fewer tiles -> a larger split-K factor -> more partials), so it is the max over the ranks'
// shard sizes, not rank 0's
size_t sharded_ws(int t, int64_t M, int64_t N, int64_t K, int world)
{
    int64_t row0, rows, R;
    size_t local = 0;
    for (int g = 0; g < world; ++g) {
        shard_geom(M, world, g, row0, rows, R);
        const size_t w = gq::plan_call(gq::shape_call(t, GQ_ACT_Q8_1, rows, N, K, true), gq::tuning()).ws_bytes();
        local = w > local ? w : local;
    }
    return gq::align_up((size_t)N * R * 2) + gq::align_up((size_t)world * N * R * 2) + local;
}

// The shapes the size queries answer (else 0): what the launch entries refuse by type, sizes or K
// alone is refused here too, before any planning divides by a block count.  Two refused
// combinations are still sized, as they always were: the fp8 variant at K % 256 != 0
// (test_abi.py::test_fp8_host_argument_checks pins gq_mmq_workspace_size_ex(Q8_0, fp8, 8, 4, 96) > 0)
// and Q5_K / Q3_K / Q2_K with fp8 activations.
bool sizable(int t, int act, int64_t M, int64_t N, int64_t K)
{
    if (!gq::known_type(t) || (act != GQ_ACT_Q8_1 && act != GQ_ACT_FP8_E4M3)) return false;
    return M >= 0 && N > 0 && K > 0 && K % gq::fmt_info(t).qk == 0;
}

// The launches of the chunked kernels (launch_plan, plan_entries): fn(m0, mc, n0, nc) per launch
// until it fails; K_SGEMM cuts rows alone.  Chunks of < 2 GiB of weights and of activations per launch
// (32-bit buffer offsets).
template <class Fn> static hipError_t for_chunks(int64_t M, int64_t N, int64_t rows, int64_t toks, Fn &&fn)
{
    hipError_t e = hipSuccess;
    for (int64_t n0 = 0; n0 < N && e == hipSuccess; n0 += toks)
        for (int64_t m0 = 0; m0 < M && e == hipSuccess; m0 += rows)
            e = fn(m0, M - m0 < rows ? M - m0 : rows, n0, N - n0 < toks ? N - n0 : toks);
    return e;
}
// a row chunk of the streaming GEMM plans its own splits
static gq::RGemmPlan sgemm_chunk_plan(const gq::Plan &p, int64_t mc, int64_t M, int64_t N, int64_t K)
{
    return mc == M ? p.rg : gq::plan_sgemm(mc, N, K, gq::tuning().sgemm_splits);
}
static gq::KItem kstream_item(const gq::Call &c, const uint8_t *A, const uint16_t *X, int64_t ldx, uint16_t *C)
{
    return gq::KItem{c.t, A, X, ldx, C, c.ldc, c.M, c.K};
}

} // namespace

extern "C" {

int gq_debug_set_tuning(const char *key, long long value)
{
    g_err.clear();
    if (gq::set_tuning(key, value) != 0)
        return fail(GQ_EINVAL, "unknown tuning key or value out of range: %s=%lld", key ? key : "(null)", value);
    return GQ_OK;
}
void gq_debug_reset_tuning(void) { gq::reset_tuning(); }

int gq_block_elems(gq_type t) { return gq::fmt_info(t).qk; }
int gq_block_bytes(gq_type t) { return gq::fmt_info(t).bytes; }
int gq_version(void) { return 105; }

unsigned int gq_debug_sync_timeouts(void) { return gq::ilc_timeouts() + gq::kstream_timeouts(); }
const char *gq_last_error(void) { return g_err.c_str(); }

// what a gq_mmq_ex call itself needs (gq_act_prepare / gq_mmq_prepared: gq_mmq_workspace_size_ex)
size_t gq_mmq_call_workspace_size(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K)
{
    if (!sizable(t, act, M, N, K)) return 0;
    return gq::plan_call(gq::shape_call(t, act, M, N, K, false), gq::tuning()).ws_bytes();
}
size_t gq_mmq_workspace_size_ex(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K)
{
    if (!sizable(t, act, M, N, K)) return 0;
    return gq::plan_call(gq::shape_call(t, act, M, N, K, true), gq::tuning()).ws_bytes();
}
size_t gq_mmq_workspace_size(gq_type t, int64_t M, int64_t N, int64_t K)
{
    return gq_mmq_workspace_size_ex(t, GQ_ACT_Q8_1, M, N, K);
}

static int check_common(gq_type t, int64_t M, int64_t N, int64_t K)
{
    if (!gq::known_type(t)) return fail(GQ_EUNSUPPORTED, "unknown gguf type %d", (int)t);
    if (M < 0 || N < 0 || K < 0)
        return fail(GQ_EINVAL, "negative size M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    const int qk = gq::fmt_info(t).qk;
    if (K % qk != 0) return fail(GQ_EINVAL, "K=%lld is not a multiple of %d", (long long)K, qk);
    return GQ_OK;
}

static int check_act(int act, int64_t K)
{
    if (act != GQ_ACT_Q8_1 && act != GQ_ACT_FP8_E4M3) return fail(GQ_EUNSUPPORTED, "unknown activation format %d", act);
    if (act == GQ_ACT_FP8_E4M3 && !gq::gemm_supported(gq::Q8_0, K))
        return fail(GQ_EUNSUPPORTED, "fp8 activations need K %% 256 == 0 (K=%lld)", (long long)K);
    return GQ_OK;
}

// The shape checks every MMQ entry starts with, in this order: the type and the sizes, the
// activation format, and the pair (Q5_K, Q3_K, Q2_K and Q4_0 run with q8_1 activations only)
static int check_mmq_shape(gq_type t, int act, int64_t M, int64_t N, int64_t K)
{
    int rc = check_common(t, M, N, K);
    if (rc != GQ_OK) return rc;
    if ((rc = check_act(act, K)) != GQ_OK) return rc;
    if (gq::q8_1_only(t) && act == GQ_ACT_FP8_E4M3)
        return fail(GQ_EUNSUPPORTED, "%s has no fp8-activation form", gq::type_info(t).name);
    return GQ_OK;
}

static int fail_workspace(const void *workspace, size_t have, size_t need, const char *pre = "")
{
    return fail(GQ_EINVAL, "%sworkspace %zu bytes < required %zu", pre, workspace ? have : (size_t)0, need);
}

using gq::carve;
using gq::Carved;

// gq_act_prepare_ex's checks of one activation tensor, in its order; item >= 0: an item of
// gq_act_prepare_grouped (named in the text).  empty: nothing to write.
static int check_prep_item(int act, const void *B, int64_t N, int64_t K, int64_t ldb, const void *workspace,
                           size_t workspace_bytes, int item, bool &empty)
{
    char pre[24] = "";
    if (item >= 0) snprintf(pre, sizeof(pre), "item %d: ", item);
    empty = false;
    if (N < 0 || K < 0) return fail(GQ_EINVAL, "%snegative size", pre);
    if (K % 32 != 0) return fail(GQ_EINVAL, "%sK=%lld is not a multiple of 32", pre, (long long)K);
    const int rc = check_act(act, K);
    if (rc != GQ_OK) return rc;
    empty = N == 0 || K == 0;
    if (empty) return GQ_OK;
    if (!B) return fail(GQ_EINVAL, "%snull activation pointer", pre);
    if (ldb < K) return fail(GQ_EINVAL, "%sldb=%lld < K=%lld", pre, (long long)ldb, (long long)K);
    const size_t need = gq::act_bytes(act, N, K);
    if (!workspace || workspace_bytes < need) return fail_workspace(workspace, workspace_bytes, need, pre);
    return GQ_OK;
}

// The activation quantizer's launches into a checked workspace.
// q8_1 forms: bit 0 = fp16 x~ (DEQ), bit 1 = int8 codes + d (I8), bit 2 = with the I8 form, s
// too (the integer skinny kernel); only the GEMM path reads them
static int prepare(int act, const void *B, int64_t N, int64_t K, int64_t ldb, void *workspace, hipStream_t s, int forms)
{
    Carved c = carve(act, workspace, N, K);
    hipError_t e = hipSuccess;
    if (act == GQ_ACT_FP8_E4M3) {
        e = gq::launch_act_quant(gq::ACT_F8DEQ, (const uint16_t *)B, ldb, N, K, c.xdeq, nullptr, nullptr, s);
    } else if (gq::use_gemv(N, K)) {
        e = gq::launch_act_quant(gq::ACT_SOA, (const uint16_t *)B, ldb, N, K, c.xq, c.xd, c.xs, s);
    } else {
        if (forms & 1) e = gq::launch_act_quant(gq::ACT_DEQ, (const uint16_t *)B, ldb, N, K, c.xdeq, nullptr, nullptr, s);
        if (e == hipSuccess && (forms & 2))
            e = gq::launch_act_quant(gq::ACT_I8, (const uint16_t *)B, ldb, N, K, c.xq, c.xd, (forms & 4) ? c.xs : nullptr, s);
    }
    if (e == hipSuccess && c.xraw)
        e = hipMemcpy2DAsync(c.xraw, (size_t)K * 2, B, (size_t)ldb * 2, (size_t)K * 2, (size_t)N, hipMemcpyDeviceToDevice, s);
    return hip_rc(e, "act_quant");
}

// The launches of a plan.  B: the caller's activations (a raw plan quantizes them in the kernel);
// every other plan reads what prepare() left in the workspace.
static int launch_plan(const gq::Call &c, const gq::Plan &p, const void *A_, const void *B, void *workspace, void *C_,
                       hipStream_t s)
{
    const int t = c.t;
    const int64_t M = c.M, N = c.N, K = c.K, ldc = c.ldc;
    const uint8_t *A = (const uint8_t *)A_;
    uint16_t *C = (uint16_t *)C_;
    const Carved w = workspace ? carve(c.act, workspace, N, K) : Carved{};
    const uint16_t *X = p.raw ? (const uint16_t *)B : w.xdeq;
    const int64_t ldx = p.raw ? c.ldb : K;
    hipError_t e = hipSuccess;
    switch (p.kernel) {
    case gq::K_NONE:
        return fail(GQ_EUNSUPPORTED, "%s: not a streaming-GEMM shape (M=%lld N=%lld K=%lld)", gq::type_info(t).name,
                    (long long)M, (long long)N, (long long)K);
    case gq::K_DECODE: // one launch: activation quantization in LDS + the weight stream
        return hip_rc(gq::launch_decode_fused(t, A, p.raw ? X : w.xraw, ldx, C, M, N, K, ldc, s, c.act == GQ_ACT_FP8_E4M3),
                      "decode");
    case gq::K_BLAS: {
        uint16_t *W = (uint16_t *)w.partials; // after the activations: fp16 W, then the BLAS workspace
        uint8_t *bws = (uint8_t *)W + gq::align_up((size_t)M * K * 2);
        const int rc = hip_rc(gq::launch_dequant(t, A, W, M, K, K, true, s), "dequant");
        if (rc != GQ_OK) return rc;
        const int brc = gq::blas_gemm(W, w.xdeq, C, M, N, K, ldc, bws, gq::blas_workspace_bytes(), s);
        if (brc != 0) return fail(GQ_EHIP, "hipBLASLt GEMM failed (code %d)", brc);
        return GQ_OK;
    }
    case gq::K_GEMV: return hip_rc(gq::launch_gemv(t, A, w.xq, w.xd, w.xs, C, M, N, K, ldc, s), "mmq");
    case gq::K_KSTREAM: {
        const gq::KItem it = kstream_item(c, A, X, ldx, C);
        return hip_rc(gq::launch_kstream(&it, 1, N, p.aq, w.partials, s), "kstream");
    }
    case gq::K_RGEMM: // (+ the split-K reduce)
        return hip_rc(gq::launch_rgemm(t, p.aq, A, X, ldx, C, w.partials, p.rg, M, N, K, ldc, s), "rgemm");
    case gq::K_SGEMM_STREAMK: {
        gq::SGroupItem it = p.item;
        it.A = A;
        it.X = w.xdeq;
        it.C = C;
        it.ldc = ldc;
        return hip_rc(gq::launch_sgemm_grouped(&it, 1, N, p.sg, w.partials, s), "sgemm");
    }
    case gq::K_SGEMM: // row chunks under the per-launch byte limit (Q5_K / Q3_K / Q2_K; the others are never cut)
        e = for_chunks(M, N, p.rows, N, [&](int64_t m0, int64_t mc, int64_t, int64_t) {
            return gq::launch_sgemm(t, A + m0 * gq::row_bytes(t, K), w.xdeq, C + m0, w.partials,
                                    sgemm_chunk_plan(p, mc, M, N, K), mc, N, K, ldc, s);
        });
        return hip_rc(e, "sgemm");
    case gq::K_SKINNY:
    case gq::K_GEMM:
        break;
    }
    if (p.raw) { // K_GEMM on the caller's activations
        gq::GemmAct x;
        x.xraw = X;
        x.ldx = ldx;
        return hip_rc(gq::launch_gemm(t, A, x, C, w.partials, p.gemm, M, N, K, ldc, s), "mmq");
    }
    e = for_chunks(M, N, p.rows, p.toks, [&](int64_t m0, int64_t mc, int64_t n0, int64_t nc) {
        const uint8_t *Ac = A + m0 * gq::row_bytes(t, K);
        uint16_t *Cc = C + n0 * ldc + m0;
        if (p.kernel == gq::K_SKINNY)
            return gq::launch_skinny(t, Ac, w.xdeq + n0 * K, Cc, gq::plan_skinny(t, mc, nc, K, gq::tuning().skinny_rg, 0), mc,
                                     nc, K, ldc, s);
        gq::GemmAct x;
        x.xdeq = w.xdeq ? w.xdeq + n0 * K : nullptr;
        x.xq = w.xq ? w.xq + n0 * K : nullptr;
        x.xd = w.xd ? w.xd + n0 : nullptr;
        x.ldd = gq::scale_ld(N);
        return gq::launch_gemm(t, Ac, x, Cc, w.partials, gq::plan_gemm(t, mc, nc, K, p.form), mc, nc, K, ldc, s);
    });
    return hip_rc(e, "mmq");
}

// launch_plan's launches as data (gq_debug_gemm_plan): the same switch, each case the kernel file's
// *_plan_info beside the launcher launch_plan calls.  Returns the new entry count.
static int plan_entries(const gq::Call &c, const gq::Plan &p, gq::GemmPlanInfo *out, int at, int max_out)
{
    const int t = c.t;
    const int64_t M = c.M, N = c.N, K = c.K;
    switch (p.kernel) {
    case gq::K_NONE:
    case gq::K_DECODE:
    case gq::K_BLAS:
    case gq::K_GEMV: return at; // (no GEMM kernel of the four files)
    case gq::K_KSTREAM: {
        const gq::KItem it = kstream_item(c, nullptr, nullptr, p.raw ? c.ldb : K, nullptr);
        return gq::kstream_plan_info(&it, 1, N, p.aq, nullptr, out, at, max_out);
    }
    case gq::K_RGEMM:
        return gq::rgemm_plan_info(t, p.aq, p.raw ? c.ldb : K, p.rg, M, N, K, out, at, max_out);
    case gq::K_SGEMM_STREAMK: return gq::sgemm_grouped_plan_info(&p.item, 1, N, p.sg, nullptr, out, at, max_out);
    case gq::K_SGEMM:
        (void)for_chunks(M, N, p.rows, N, [&](int64_t, int64_t mc, int64_t, int64_t) {
            at = gq::sgemm_plan_info(t, sgemm_chunk_plan(p, mc, M, N, K), mc, N, K, out, at, max_out);
            return hipSuccess;
        });
        return at;
    case gq::K_SKINNY:
    case gq::K_GEMM: break;
    }
    if (p.raw) return gq::gemm_plan_info(t, p.gemm, M, N, K, out, at, max_out);
    (void)for_chunks(M, N, p.rows, p.toks, [&](int64_t, int64_t mc, int64_t, int64_t nc) {
        at = p.kernel == gq::K_SKINNY
                 ? gq::skinny_plan_info(t, gq::plan_skinny(t, mc, nc, K, gq::tuning().skinny_rg, 0), mc, nc, K, out, at, max_out)
                 : gq::gemm_plan_info(t, gq::plan_gemm(t, mc, nc, K, p.form), mc, nc, K, out, at, max_out);
        return hipSuccess;
    });
    return at;
}

// gq_mmq_ex runs a raw call's own plan when it is one launch on the caller's activations (or refused);
// every other raw call is act_quant + the prepared call's plan (Plan::raw)
static bool runs_own_plan(const gq::Plan &p) { return p.raw || p.kernel == gq::K_NONE; }

// gq_mmq_prepared_ex after the shape checks
static int run_prepared(gq_type t, int act, const void *A, void *workspace, size_t workspace_bytes, void *C, int64_t M,
                        int64_t N, int64_t K, int64_t ldc, hipStream_t s)
{
    if (!A || !C || !workspace) return fail(GQ_EINVAL, "null pointer (A=%p C=%p workspace=%p)", A, C, workspace);
    if (ldc < M) return fail(GQ_EINVAL, "ldc=%lld < M=%lld", (long long)ldc, (long long)M);
    const gq::Call c{t, act, M, N, K, true, K, ldc, true, gq::c8(C)};
    const gq::Plan p = gq::plan_call(c, gq::tuning());
    if (workspace_bytes < p.ws_bytes()) return fail_workspace(workspace, workspace_bytes, p.ws_bytes());
    return launch_plan(c, p, A, nullptr, workspace, C, s);
}

int gq_mmq_ex(gq_type t, gq_act act, const void *A, const void *B, void *C, int64_t M, int64_t N, int64_t K,
              int64_t ldb, int64_t ldc, void *workspace, size_t workspace_bytes, void *stream)
{
    g_err.clear();
    int rc = check_mmq_shape(t, act, M, N, K);
    if (rc != GQ_OK) return rc;
    if (M == 0 || N == 0) return GQ_OK;
    if (K == 0) return fail(GQ_EINVAL, "K must be positive");
    if (!A || !B || !C) return fail(GQ_EINVAL, "null pointer (A=%p B=%p C=%p)", A, B, C);
    if (ldc < M) return fail(GQ_EINVAL, "ldc=%lld < M=%lld", (long long)ldc, (long long)M);
    if (ldb < K) return fail(GQ_EINVAL, "ldb=%lld < K=%lld", (long long)ldb, (long long)K);
    const gq::Call c{t, act, M, N, K, false, ldb, ldc, ldb % 8 == 0 && ((uintptr_t)B & 15) == 0, gq::c8(C)};
    const gq::Plan p = gq::plan_call(c, gq::tuning());
    const size_t need = p.ws_bytes();
    if (need && (!workspace || workspace_bytes < need)) return fail_workspace(workspace, workspace_bytes, need);
    if (runs_own_plan(p)) return launch_plan(c, p, A, B, workspace, C, (hipStream_t)stream); // (or refused)
    // act_quant, then the prepared call (its own plan: see Plan::raw)
    rc = prepare(act, B, N, K, ldb, workspace, (hipStream_t)stream, p.forms);
    if (rc != GQ_OK) return rc;
    return run_prepared(t, act, A, workspace, workspace_bytes, C, M, N, K, ldc, (hipStream_t)stream);
}

int gq_mmq(gq_type t, const void *A, const void *B, void *C, int64_t M, int64_t N, int64_t K, int64_t ldb,
           int64_t ldc, void *workspace, size_t workspace_bytes, void *stream)
{
    return gq_mmq_ex(t, GQ_ACT_Q8_1, A, B, C, M, N, K, ldb, ldc, workspace, workspace_bytes, stream);
}

int gq_act_prepare_ex(gq_act act, const void *B, int64_t N, int64_t K, int64_t ldb, void *workspace,
                      size_t workspace_bytes, void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_prep_item(act, B, N, K, ldb, workspace, workspace_bytes, -1, empty);
    if (rc != GQ_OK || empty) return rc;
    // the weight type is not known here: write every form a later gq_mmq_prepared may read
    // (the int8 form only when Q8_0 would use it)
    return prepare(act, B, N, K, ldb, workspace, (hipStream_t)stream, gq::use_i8(GQ_Q8_0, N, K, gq::tuning()) ? 3 : 1);
}

int gq_act_prepare(const void *B, int64_t N, int64_t K, int64_t ldb, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    return gq_act_prepare_ex(GQ_ACT_Q8_1, B, N, K, ldb, workspace, workspace_bytes, stream);
}

int gq_act_prepare_grouped(gq_act act, const gq_prep_item *items, int n, void *stream)
{
    g_err.clear();
    if (n < 0 || (n > 0 && !items)) return fail(GQ_EINVAL, "bad item list (n=%d, items=%p)", n, (const void *)items);
    // every item checked first: a bad item launches nothing
    for (int i = 0; i < n; ++i) {
        const gq_prep_item &it = items[i];
        bool empty;
        const int rc = check_prep_item(act, it.B, it.N, it.K, it.ldb, it.workspace, it.workspace_bytes, i, empty);
        if (rc != GQ_OK) return rc;
    }
    const hipStream_t s = (hipStream_t)stream;
    gq::DeqSeg segs[gq::kMaxDeqSegs];
    int ns = 0;
    auto flush = [&]() -> int {
        if (ns == 0) return GQ_OK;
        const hipError_t e = gq::launch_act_quant_deq_grouped(segs, ns, s, act == GQ_ACT_FP8_E4M3 ? gq::ACT_F8DEQ : gq::ACT_DEQ);
        ns = 0;
        return hip_rc(e, "grouped act_quant");
    };
    for (int i = 0; i < n; ++i) {
        const gq_prep_item &it = items[i];
        const int64_t N = it.N, K = it.K;
        if (N == 0 || K == 0) continue;
        int rc;
        const bool i8 = gq::use_i8(GQ_Q8_0, N, K, gq::tuning());
        if (act == GQ_ACT_Q8_1 && (gq::use_gemv(N, K) || i8)) { // its own launch(es), as gq_act_prepare_ex
            if ((rc = prepare(act, it.B, N, K, it.ldb, it.workspace, s, i8 ? 3 : 1)) != GQ_OK) return rc;
            continue;
        }
        if (ns == gq::kMaxDeqSegs && (rc = flush()) != GQ_OK) return rc;
        // the fp16 x~ form sits at the front of the workspace (carve)
        const Carved c = carve(act, it.workspace, N, K);
        segs[ns++] = gq::DeqSeg{(const uint16_t *)it.B, it.ldb, N, K, c.xdeq, 0};
        if (c.xraw) { // (fp8 at 1-2 tokens: the decode's copy, as prepare())
            const hipError_t e = hipMemcpy2DAsync(c.xraw, (size_t)K * 2, it.B, (size_t)it.ldb * 2, (size_t)K * 2,
                                                  (size_t)N, hipMemcpyDeviceToDevice, s);
            if (e != hipSuccess) return fail(GQ_EHIP, "HIP copy failed (grouped act_quant): %s", hipGetErrorString(e));
        }
    }
    return flush();
}

int gq_mmq_prepared_ex(gq_type t, gq_act act, const void *A, void *workspace, size_t workspace_bytes, void *C,
                       int64_t M, int64_t N, int64_t K, int64_t ldc, void *stream)
{
    g_err.clear();
    const int rc = check_mmq_shape(t, act, M, N, K);
    if (rc != GQ_OK) return rc;
    if (M == 0 || N == 0) return GQ_OK;
    if (K == 0) return fail(GQ_EINVAL, "K must be positive");
    return run_prepared(t, act, A, workspace, workspace_bytes, C, M, N, K, ldc, (hipStream_t)stream);
}

int gq_mmq_prepared(gq_type t, const void *A, void *workspace, size_t workspace_bytes, void *C, int64_t M, int64_t N,
                    int64_t K, int64_t ldc, void *stream)
{
    return gq_mmq_prepared_ex(t, GQ_ACT_Q8_1, A, workspace, workspace_bytes, C, M, N, K, ldc, stream);
}

int gq_dequantize(gq_type t, const void *A, void *W, int64_t M, int64_t K, int64_t ldw, void *stream)
{
    g_err.clear();
    int rc = check_common(t, M, 1, K);
    if (rc != GQ_OK) return rc;
    if (M == 0 || K == 0) return GQ_OK;
    if (!A || !W) return fail(GQ_EINVAL, "null pointer");
    if (ldw < K) return fail(GQ_EINVAL, "ldw=%lld < K=%lld", (long long)ldw, (long long)K);
    return hip_rc(gq::launch_dequant(t, (const uint8_t *)A, (uint16_t *)W, M, K, ldw, false, (hipStream_t)stream));
}

int gq_quantize_q8_1(const void *X, void *Y, int64_t rows, int64_t K, int64_t ldx, void *stream)
{
    g_err.clear();
    if (rows < 0 || K < 0) return fail(GQ_EINVAL, "negative size");
    if (K % 32 != 0) return fail(GQ_EINVAL, "K=%lld is not a multiple of 32", (long long)K);
    if (rows == 0 || K == 0) return GQ_OK;
    if (!X || !Y) return fail(GQ_EINVAL, "null pointer");
    if (ldx < K) return fail(GQ_EINVAL, "ldx=%lld < K=%lld", (long long)ldx, (long long)K);
    return hip_rc(gq::launch_act_quant(gq::ACT_AOS, (const uint16_t *)X, ldx, rows, K, Y, nullptr, nullptr,
                                       (hipStream_t)stream));
}

int gq_quantize_weights(gq_type t, const void *X, void *Y, int64_t n, void *stream)
{
    g_err.clear();
    const gq::TypeInfo &ti = gq::type_info(t);
    if (!gq::known_type(t)) return fail(GQ_EUNSUPPORTED, "unknown gguf type %d", (int)t);
    if (ti.quant_kind < 0)
        return fail(GQ_EUNSUPPORTED, "%s has no device quantizer (gq_quantize_%s on the host)", ti.name, ti.lname);
    if (n < 0) return fail(GQ_EINVAL, "negative size");
    const int qk = gq::fmt_info(t).qk;
    if (n % qk != 0) return fail(GQ_EINVAL, "n=%lld is not a multiple of %d", (long long)n, qk);
    if (n == 0) return GQ_OK;
    if (!X || !Y) return fail(GQ_EINVAL, "null pointer");
    return hip_rc(gq::launch_quant_blocks(ti.quant_kind, X, Y, n / qk, (hipStream_t)stream), "weight quantizer");
}

int gq_quantize_fp8(const void *X, void *codes, void *scales, int64_t rows, int64_t K, int64_t ldx, void *stream)
{
    g_err.clear();
    if (rows < 0 || K < 0) return fail(GQ_EINVAL, "negative size");
    if (K % 32 != 0) return fail(GQ_EINVAL, "K=%lld is not a multiple of 32", (long long)K);
    if (rows == 0 || K == 0) return GQ_OK;
    if (!X || !codes || !scales) return fail(GQ_EINVAL, "null pointer");
    if (ldx < K) return fail(GQ_EINVAL, "ldx=%lld < K=%lld", (long long)ldx, (long long)K);
    return hip_rc(gq::launch_act_quant(gq::ACT_F8, (const uint16_t *)X, ldx, rows, K, codes, scales, nullptr,
                                       (hipStream_t)stream));
}

int gq_shard_rows(int64_t M, int world, int rank, int64_t *row0, int64_t *rows, int64_t *R)
{
    g_err.clear();
    if (M < 0 || world < 1 || rank < 0 || rank >= world)
        return fail(GQ_EINVAL, "bad shard (M=%lld world=%d rank=%d)", (long long)M, world, rank);
    if (!row0 || !rows || !R) return fail(GQ_EINVAL, "null output pointer");
    shard_geom(M, world, rank, *row0, *rows, *R);
    return GQ_OK;
}

int gq_assemble_shards(const void *gathered, void *C, int world, int64_t N, int64_t R, int64_t M, int64_t ldc,
                       void *stream)
{
    g_err.clear();
    if (world < 1 || N < 0 || R < 0 || M < 0) return fail(GQ_EINVAL, "negative size or world < 1");
    if (M > (int64_t)world * R) return fail(GQ_EINVAL, "M=%lld > world*R=%lld", (long long)M, (long long)world * R);
    if (R % 8 != 0) return fail(GQ_EINVAL, "R=%lld is not a multiple of 8", (long long)R);
    if (ldc < M) return fail(GQ_EINVAL, "ldc=%lld < M=%lld", (long long)ldc, (long long)M);
    if (N == 0 || M == 0) return GQ_OK;
    if (!gathered || !C) return fail(GQ_EINVAL, "null pointer");
    return hip_rc(launch_assemble((const uint16_t *)gathered, (uint16_t *)C, N, R, M, ldc, (hipStream_t)stream), "assemble");
}

size_t gq_mmq_sharded_workspace_size(gq_type t, int64_t M, int64_t N, int64_t K, int world)
{
    if (!sizable(t, GQ_ACT_Q8_1, M, N, K) || world < 1) return 0;
    return sharded_ws(t, M, N, K, world);
}

int gq_mmq_grouped(const gq_group_item *items, int n, int64_t N, void *stream)
{
    return gq_mmq_grouped_ex(GQ_ACT_Q8_1, items, n, N, stream);
}

// gq_mmq_grouped_ex at 5..32 tokens (fp8: 3..32): an item of the K-chunked stream's one launch (the
// grouped launch's own route: the stream wherever it applies, GQ_KSTREAM=0 refuses; no K ranges; rows
// the in-kernel quantizer can load)
static bool grouped_ex_kstream_item(const gq::DecodeItem &d, gq_act act, int64_t N)
{
    return gq::grouped_kstream_item(d.fmt, act, d.M, N, d.K, d.ldx, d.ldc, d.C, false, gq::tuning()) &&
           gq::kstream_splits(d.K) <= 1 && d.ldx % 8 == 0 && ((uintptr_t)d.X & 15) == 0;
}
static bool grouped_ex_is_kstream(gq_act act, int64_t N) { return N >= (act == GQ_ACT_FP8_E4M3 ? 3 : 5); }

int gq_mmq_grouped_ex(gq_act act, const gq_group_item *items, int n, int64_t N, void *stream)
{
    g_err.clear();
    const bool fp8 = act == GQ_ACT_FP8_E4M3;
    if (n < 0 || (n > 0 && !items)) return fail(GQ_EINVAL, "bad item list (n=%d, items=%p)", n, (const void *)items);
    if (N < 0) return fail(GQ_EINVAL, "negative N");
    gq::DecodeItem di[16];
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const gq_group_item &it = items[i];
        const int rc = check_mmq_shape(it.type, act, it.M, N, it.K);
        if (rc != GQ_OK) return rc;
        if (it.M == 0 || N == 0) continue;
        if (it.K == 0) return fail(GQ_EINVAL, "item %d: K must be positive", i);
        if (!it.A || !it.B || !it.C) return fail(GQ_EINVAL, "item %d: null pointer", i);
        if (it.ldb < it.K) return fail(GQ_EINVAL, "item %d: ldb=%lld < K=%lld", i, (long long)it.ldb, (long long)it.K);
        if (it.ldc < it.M) return fail(GQ_EINVAL, "item %d: ldc=%lld < M=%lld", i, (long long)it.ldc, (long long)it.M);
        if (m == 16) return fail(GQ_EUNSUPPORTED, "more than 16 items");
        di[m++] = gq::DecodeItem{it.type, (const uint8_t *)it.A, (const uint16_t *)it.B, it.ldb, (uint16_t *)it.C,
                                 it.ldc, it.M, it.K};
    }
    if (m == 0) return GQ_OK;
    // (3..4 q8_1 tokens stay on the grouped decode: the stream for the K <= 4096 items with the
    // long-K item on its own measured 13% slower on the 7B layer, profiles/r06/kstream_rawg3_ab.txt)
    if (grouped_ex_is_kstream(act, N)) {
        // 5..32 tokens (fp8: 3..32): the K-chunked streaming MMQ, every item in one launch
        gq::KItem ki[16];
        for (int i = 0; i < m; ++i) {
            const gq::DecodeItem &d = di[i];
            if (!grouped_ex_kstream_item(d, act, N))
                return fail(GQ_EUNSUPPORTED, "item %d (%s): not a grouped K-chunked-stream shape (N=%lld, M=%lld, K=%lld)", i,
                            gq::type_info(d.fmt).name, (long long)N, (long long)d.M, (long long)d.K);
            ki[i] = gq::KItem{d.fmt, d.A, d.X, d.ldx, d.C, d.ldc, d.M, d.K};
        }
        // (no K ranges)
        return hip_rc(gq::launch_kstream(ki, m, N, fp8 ? 2 : 1, nullptr, (hipStream_t)stream), "grouped kstream");
    }
    if (!gq::decode_grouped_ok(di, m, N, fp8))
        return fail(GQ_EUNSUPPORTED, "not a grouped-decode shape (N=%lld; N <= %d and every item a one-launch decode)",
                    (long long)N, fp8 ? 2 : 4);
    hipError_t e = gq::launch_decode_grouped(di, m, N, (hipStream_t)stream, fp8);
    if (e == hipErrorInvalidValue) return fail(GQ_EUNSUPPORTED, "grouped decode: more than 16 parts");
    return hip_rc(e, "grouped decode");
}

// The checks gq_mmq_id and gq_mmq_id_sorted share, in their order.  empty: nothing to compute.
static int check_id_args(gq_type t, const void *A, const int32_t *ids, const void *B, const void *C, int64_t E, int64_t M,
                         int64_t N, int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc, bool &empty)
{
    empty = false;
    const int rc = check_mmq_shape(t, GQ_ACT_Q8_1, M, N, K);
    if (rc != GQ_OK) return rc;
    if (S < 0 || E < 0) return fail(GQ_EINVAL, "negative size S=%lld E=%lld", (long long)S, (long long)E);
    empty = M == 0 || N == 0 || S == 0;
    if (empty) return GQ_OK;
    if (K == 0) return fail(GQ_EINVAL, "K must be positive");
    if (E == 0) return fail(GQ_EINVAL, "E must be positive");
    if (!A || !ids || !B || !C) return fail(GQ_EINVAL, "null pointer (A=%p ids=%p B=%p C=%p)", A, (const void *)ids, B, C);
    if (ldc < M) return fail(GQ_EINVAL, "ldc=%lld < M=%lld", (long long)ldc, (long long)M);
    if (ldb < K) return fail(GQ_EINVAL, "ldb=%lld < K=%lld", (long long)ldb, (long long)K);
    if (ldb_slot != 0 && ldb_slot < K)
        return fail(GQ_EINVAL, "ldb_slot=%lld is neither 0 (shared row) nor >= K=%lld", (long long)ldb_slot, (long long)K);
    return GQ_OK;
}

int gq_mmq_id(gq_type t, const void *A, const int32_t *ids, const void *B, void *C, int64_t E, int64_t M, int64_t N,
              int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc, void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_id_args(t, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc, empty);
    if (rc != GQ_OK || empty) return rc;
    // (activation rows: no alignment beyond fp16's -- the decode prologue's 16-byte loads take any
    // address, and gq_mmq_ex's fused-decode route asks none)
    if (N > gq::kMaxIdPairs || S > gq::kMaxIdPairs || !gq::decode_id_ok(t, M, N * S, K) || E > INT32_MAX)
        return fail(GQ_EUNSUPPORTED,
                    "not an expert-indexed decode shape (N=%lld x S=%lld pairs, at most %d; K=%lld must fit the "
                    "one-token decode; one expert < 2 GiB)",
                    (long long)N, (long long)S, gq::kMaxIdPairs, (long long)K);
    return hip_rc(gq::launch_decode_id(t, (const uint8_t *)A, ids, (const uint16_t *)B, (uint16_t *)C, E, M, N, S, K, ldb,
                                       ldb_slot, ldc, (hipStream_t)stream),
                  "id decode");
}

int gq_mmq_id_glu(gq_type t, const void *A_gate, const void *A_up, const int32_t *ids, const void *B, void *H, int64_t E,
                  int64_t M, int64_t N, int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldh, void *stream)
{
    g_err.clear();
    bool empty;
    // gq_mmq_id's checks in its order (a null A_up counts as a null A)
    const int rc = check_id_args(t, A_up ? A_gate : nullptr, ids, B, H, E, M, N, S, K, ldb, ldb_slot, ldh, empty);
    if (rc != GQ_OK || empty) return rc;
    if (N > gq::kMaxIdPairs || S > gq::kMaxIdPairs || !gq::decode_id_glu_ok(t, M, N * S, K) || E > INT32_MAX)
        return fail(GQ_EUNSUPPORTED,
                    "not an expert-indexed gate/up shape (N=%lld x S=%lld pairs, at most %d; K=%lld must fit the "
                    "one-token decode; one expert < 2 GiB)",
                    (long long)N, (long long)S, gq::kMaxIdPairs, (long long)K);
    return hip_rc(gq::launch_decode_id_glu(t, (const uint8_t *)A_gate, (const uint8_t *)A_up, ids, (const uint16_t *)B,
                                           (uint16_t *)H, E, M, N, S, K, ldb, ldb_slot, ldh, (hipStream_t)stream),
                  "id glu decode");
}

int gq_mmq_glu(gq_type t, const void *A_gate, const void *A_up, const void *B, void *H, int64_t M, int64_t N, int64_t K,
               int64_t ldb, int64_t ldh, void *stream)
{
    g_err.clear();
    const int rc = check_mmq_shape(t, GQ_ACT_Q8_1, M, N, K);
    if (rc != GQ_OK) return rc;
    if (M == 0 || N == 0) return GQ_OK;
    if (K == 0) return fail(GQ_EINVAL, "K must be positive");
    if (!A_gate || !A_up || !B || !H)
        return fail(GQ_EINVAL, "null pointer (A_gate=%p A_up=%p B=%p H=%p)", A_gate, A_up, B, H);
    if (ldb < K) return fail(GQ_EINVAL, "ldb=%lld < K=%lld", (long long)ldb, (long long)K);
    if (ldh < M) return fail(GQ_EINVAL, "ldh=%lld < M=%lld", (long long)ldh, (long long)M);
    // gq_mmq's own route for the shape (the one-launch decode on the caller's activations), then the
    // GLU form's limits
    const gq::Plan p = gq::plan_call(gq::shape_call(t, GQ_ACT_Q8_1, M, N, K, false), gq::tuning());
    if (N > gq::kGluMaxTokens || p.kernel != gq::K_DECODE || !p.raw || !gq::decode_glu_ok(t, M, N, K))
        return fail(GQ_EUNSUPPORTED,
                    "not a dense gate/up decode shape (N=%lld, at most %d; gq_mmq's route for M=%lld K=%lld must be the "
                    "one-launch decode; a matrix < 2 GiB; a kernel without spills whose g stash fits LDS)",
                    (long long)N, gq::kGluMaxTokens, (long long)M, (long long)K);
    return hip_rc(gq::launch_decode_glu(t, (const uint8_t *)A_gate, (const uint8_t *)A_up, (const uint16_t *)B, ldb,
                                        (uint16_t *)H, M, N, K, ldh, (hipStream_t)stream),
                  "glu decode");
}

int gq_moe_combine_shared(const void *D, const void *W, int w_is_f32, const void *Dsh, int64_t ldsh, const float *gate,
                          void *Y, int64_t N, int64_t S, int64_t M, int64_t ldd, int64_t ldy, void *stream)
{
    g_err.clear();
    if (N < 0 || S < 0 || M < 0) return fail(GQ_EINVAL, "negative size N=%lld S=%lld M=%lld", (long long)N, (long long)S, (long long)M);
    if (S == 0) return fail(GQ_EINVAL, "S must be positive: with a shared term an empty slot sum is not a no-op");
    if (N == 0 || M == 0) return GQ_OK;
    if (!D || !W || !Dsh || !Y) return fail(GQ_EINVAL, "null pointer (D=%p W=%p Dsh=%p Y=%p)", D, W, Dsh, Y);
    if (ldd < M) return fail(GQ_EINVAL, "ldd=%lld < M=%lld", (long long)ldd, (long long)M);
    if (ldsh < M) return fail(GQ_EINVAL, "ldsh=%lld < M=%lld", (long long)ldsh, (long long)M);
    if (ldy < M) return fail(GQ_EINVAL, "ldy=%lld < M=%lld", (long long)ldy, (long long)M);
    if (S > gq::kMaxIdPairs || M > INT32_MAX)
        return fail(GQ_EUNSUPPORTED, "not a combine shape (S=%lld, at most %d; M=%lld < 2^31)", (long long)S, gq::kMaxIdPairs,
                    (long long)M);
    return hip_rc(gq::launch_moe_combine_shared((const uint16_t *)D, W, w_is_f32 != 0, (const uint16_t *)Dsh, ldsh, gate,
                                                (uint16_t *)Y, N, S, M, ldd, ldy, (hipStream_t)stream),
                  "moe combine shared");
}

int gq_moe_combine(const void *D, const void *W, int w_is_f32, void *Y, int64_t N, int64_t S, int64_t M, int64_t ldd,
                   int64_t ldy, void *stream)
{
    g_err.clear();
    if (N < 0 || S < 0 || M < 0) return fail(GQ_EINVAL, "negative size N=%lld S=%lld M=%lld", (long long)N, (long long)S, (long long)M);
    if (N == 0 || S == 0 || M == 0) return GQ_OK;
    if (!D || !W || !Y) return fail(GQ_EINVAL, "null pointer (D=%p W=%p Y=%p)", D, W, Y);
    if (ldd < M) return fail(GQ_EINVAL, "ldd=%lld < M=%lld", (long long)ldd, (long long)M);
    if (ldy < M) return fail(GQ_EINVAL, "ldy=%lld < M=%lld", (long long)ldy, (long long)M);
    if (S > gq::kMaxIdPairs || M > INT32_MAX)
        return fail(GQ_EUNSUPPORTED, "not a combine shape (S=%lld, at most %d; M=%lld < 2^31)", (long long)S, gq::kMaxIdPairs,
                    (long long)M);
    return hip_rc(gq::launch_moe_combine((const uint16_t *)D, W, w_is_f32 != 0, (uint16_t *)Y, N, S, M, ldd, ldy,
                                         (hipStream_t)stream),
                  "moe combine");
}

// The checks gq_moe_topk and gq_moe_route share, in their order; route: gq_moe_route's Wr, X, ldx
// and H are checked beside their counterparts (topk passes route = false).  empty: N == 0.
static int check_route_args(bool route, const void *Wr, const void *X, int64_t ldx, int64_t H, const float *logits,
                            int64_t ldl, const float *bias, int func, const int32_t *ids, const void *W, int64_t N, int64_t E,
                            int64_t S, bool &empty)
{
    empty = false;
    if (N < 0 || E < 0 || S < 0 || (route && H < 0))
        return fail(GQ_EINVAL, "negative size N=%lld E=%lld S=%lld H=%lld", (long long)N, (long long)E, (long long)S,
                    (long long)(route ? H : 0));
    empty = N == 0;
    if (empty) return GQ_OK;
    if (route && (!Wr || !X)) return fail(GQ_EINVAL, "null pointer (Wr=%p X=%p)", Wr, X);
    if (!logits || !ids || !W) return fail(GQ_EINVAL, "null pointer (logits=%p ids=%p W=%p)", (const void *)logits, (const void *)ids, W);
    if (ldl < E) return fail(GQ_EINVAL, "ldl=%lld < E=%lld", (long long)ldl, (long long)E);
    if (route && ldx < H) return fail(GQ_EINVAL, "ldx=%lld < H=%lld", (long long)ldx, (long long)H);
    if (func != 0 && func != 1) return fail(GQ_EINVAL, "func=%d is neither 0 (softmax) nor 1 (sigmoid)", func);
    if (func == 0 && bias) return fail(GQ_EINVAL, "a selection bias goes with sigmoid gating (func 1) only");
    if (!gq::moe_topk_ok(E, S))
        return fail(GQ_EUNSUPPORTED, "not a router shape (1 <= S=%lld <= E=%lld, E at most %d, S at most %d)", (long long)S,
                    (long long)E, gq::kMaxSortExperts, gq::kMaxIdPairs);
    return GQ_OK;
}

int gq_moe_topk(const float *logits, int64_t ldl, const float *bias, int func, int norm, float scale, int32_t *ids, void *W,
                int w_is_f32, int64_t N, int64_t E, int64_t S, void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_route_args(false, nullptr, nullptr, 0, 0, logits, ldl, bias, func, ids, W, N, E, S, empty);
    if (rc != GQ_OK || empty) return rc;
    return hip_rc(gq::launch_moe_topk(logits, ldl, bias, func, norm != 0, scale, ids, W, w_is_f32 != 0, N, E, S,
                                      (hipStream_t)stream),
                  "moe topk");
}

int gq_moe_route(const void *Wr, int wr_is_f16, const void *X, int64_t ldx, float *logits, int64_t ldl, const float *bias,
                 int func, int norm, float scale, int32_t *ids, void *W, int w_is_f32, int64_t N, int64_t E, int64_t H,
                 int64_t S, void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_route_args(true, Wr, X, ldx, H, logits, ldl, bias, func, ids, W, N, E, S, empty);
    if (rc != GQ_OK || empty) return rc;
    if (!gq::moe_logits_ok(N, H))
        return fail(GQ_EUNSUPPORTED,
                    "not a device router product (N=%lld, at most %d; H=%lld %% 32 == 0): multiply outside and call "
                    "gq_moe_topk",
                    (long long)N, gq::kMaxRouteTokens, (long long)H);
    const hipError_t e = gq::launch_moe_logits(Wr, wr_is_f16 != 0, (const uint16_t *)X, ldx, logits, ldl, N, E, H,
                                               (hipStream_t)stream);
    if (e != hipSuccess) return hip_rc(e, "moe logits");
    return hip_rc(gq::launch_moe_topk(logits, ldl, bias, func, norm != 0, scale, ids, W, w_is_f32 != 0, N, E, S,
                                      (hipStream_t)stream),
                  "moe topk");
}

// The byte range [lo, hi) of an fp16 (N, K) tensor with rows ld elements apart (N, K >= 1)
struct ByteRange {
    uintptr_t lo, hi;
};
static ByteRange rows_range(const void *p, int64_t N, int64_t K, int64_t ld)
{
    return {(uintptr_t)p, (uintptr_t)p + (size_t)((N - 1) * ld + K) * 2};
}
static bool overlaps(ByteRange a, ByteRange b) { return a.lo < b.hi && b.lo < a.hi; }

// gq_rmsnorm's and gq_rmsnorm_prepare's checks, in this order (prep: with the workspace, which
// needs `need` bytes).  empty: nothing to write.
static int check_norm_args(bool prep, const void *X, const void *R, const void *H, const float *w, float eps, const void *Y,
                           int64_t N, int64_t K, int64_t ldx, int64_t ldr, int64_t ldh, int64_t ldy, const void *workspace,
                           size_t workspace_bytes, bool &empty)
{
    empty = false;
    if (N < 0 || K < 0) return fail(GQ_EINVAL, "negative size N=%lld K=%lld", (long long)N, (long long)K);
    if (K % 32 != 0) return fail(GQ_EINVAL, "K=%lld is not a multiple of 32", (long long)K);
    if (!(eps >= 0.f) || eps == INFINITY) return fail(GQ_EINVAL, "eps=%g is not a finite value >= 0", (double)eps);
    empty = N == 0 || K == 0;
    if (empty) return GQ_OK;
    if (!X || !w) return fail(GQ_EINVAL, "null pointer (X=%p w=%p)", X, (const void *)w);
    if (!prep && !Y) return fail(GQ_EINVAL, "null pointer (Y=%p)", Y);
    if (ldx < K) return fail(GQ_EINVAL, "ldx=%lld < K=%lld", (long long)ldx, (long long)K);
    if (R && ldr < K) return fail(GQ_EINVAL, "ldr=%lld < K=%lld", (long long)ldr, (long long)K);
    if (H && ldh < K) return fail(GQ_EINVAL, "ldh=%lld < K=%lld", (long long)ldh, (long long)K);
    if (Y && ldy < K) return fail(GQ_EINVAL, "ldy=%lld < K=%lld", (long long)ldy, (long long)K);
    const size_t need = prep ? gq::act_bytes(GQ_ACT_Q8_1, N, K) : 0;
    if (prep && (!workspace || workspace_bytes < need)) return fail_workspace(workspace, workspace_bytes, need);
    // H may BE X or R (the in-place residual update); any other overlap of an output with an input
    // or with another output would have one row's stores race another row's loads
    const ByteRange rx = rows_range(X, N, K, ldx), rr = R ? rows_range(R, N, K, ldr) : ByteRange{0, 0},
                    rh = H ? rows_range(H, N, K, ldh) : ByteRange{0, 0}, ry = Y ? rows_range(Y, N, K, ldy) : ByteRange{0, 0},
                    rw = prep ? ByteRange{(uintptr_t)workspace, (uintptr_t)workspace + need} : ByteRange{0, 0},
                    rg = {(uintptr_t)w, (uintptr_t)w + (size_t)K * 4};
    if (H && !(H == X && ldh == ldx) && overlaps(rh, rx)) return fail(GQ_EINVAL, "H overlaps X without being X (same base and stride)");
    if (H && R && !(H == R && ldh == ldr) && overlaps(rh, rr)) return fail(GQ_EINVAL, "H overlaps R without being R (same base and stride)");
    if (H && overlaps(rh, rg)) return fail(GQ_EINVAL, "H overlaps w");
    if (Y && (overlaps(ry, rx) || (R && overlaps(ry, rr)) || (H && overlaps(ry, rh)) || overlaps(ry, rg)))
        return fail(GQ_EINVAL, "Y overlaps X, R, H or w");
    if (prep && (overlaps(rw, rx) || (R && overlaps(rw, rr)) || (H && overlaps(rw, rh)) || (Y && overlaps(rw, ry)) || overlaps(rw, rg)))
        return fail(GQ_EINVAL, "the workspace overlaps X, R, H, Y or w");
    if (N > INT32_MAX) return fail(GQ_EUNSUPPORTED, "N=%lld: one workgroup per row, N < 2^31", (long long)N);
    return GQ_OK;
}

static gq::NormArgs norm_args(const void *X, const void *R, void *H, const float *w, float eps, void *Y, int64_t K, int64_t ldx,
                              int64_t ldr, int64_t ldh, int64_t ldy)
{
    gq::NormArgs a{};
    a.X = (const uint16_t *)X, a.R = (const uint16_t *)R, a.H = (uint16_t *)H, a.Y = (uint16_t *)Y;
    a.w = w, a.eps = eps, a.K = K, a.ldx = ldx, a.ldr = ldr, a.ldh = ldh, a.ldy = ldy;
    return a;
}

int gq_rmsnorm(const void *X, const void *R, void *H, const float *w, float eps, void *Y, int64_t N, int64_t K, int64_t ldx,
               int64_t ldr, int64_t ldh, int64_t ldy, void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_norm_args(false, X, R, H, w, eps, Y, N, K, ldx, ldr, ldh, ldy, nullptr, 0, empty);
    if (rc != GQ_OK || empty) return rc;
    return hip_rc(gq::launch_rmsnorm(norm_args(X, R, H, w, eps, Y, K, ldx, ldr, ldh, ldy), N, (hipStream_t)stream), "rmsnorm");
}

int gq_rmsnorm_prepare(const void *X, const void *R, void *H, const float *w, float eps, void *Y, int64_t N, int64_t K,
                       int64_t ldx, int64_t ldr, int64_t ldh, int64_t ldy, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    g_err.clear();
    bool empty;
    const int rc = check_norm_args(true, X, R, H, w, eps, Y, N, K, ldx, ldr, ldh, ldy, workspace, workspace_bytes, empty);
    if (rc != GQ_OK || empty) return rc;
    gq::NormArgs a = norm_args(X, R, H, w, eps, Y, K, ldx, ldr, ldh, ldy);
    if (gq::use_i8(GQ_Q8_0, N, K, gq::tuning())) {
        // gq_act_prepare writes the int8 form too: the norm into Y, then its launches on Y
        if (!Y)
            return fail(GQ_EUNSUPPORTED, "the int8 GEMM form (GQ_GEMM_I8) is written by gq_act_prepare: pass Y, or call "
                                         "gq_rmsnorm and gq_act_prepare");
        const hipError_t e = gq::launch_rmsnorm(a, N, (hipStream_t)stream);
        if (e != hipSuccess) return hip_rc(e, "rmsnorm");
        return prepare(GQ_ACT_Q8_1, Y, N, K, ldy, workspace, (hipStream_t)stream, 3);
    }
    const Carved c = carve(GQ_ACT_Q8_1, workspace, N, K);
    if (gq::use_gemv(N, K)) a.xq = c.xq, a.xd = c.xd, a.xs = c.xs, a.xraw = c.xraw;
    else a.xdeq = c.xdeq;
    return hip_rc(gq::launch_rmsnorm(a, N, (hipStream_t)stream), "rmsnorm");
}

// gq_mmq_id_sorted's shape limits (GQ_EUNSUPPORTED beyond them), or the plan
static gq::SortedPlan sorted_plan(gq_type t, int64_t E, int64_t M, int64_t N, int64_t S, int64_t K)
{
    gq::SortedPlan none;
    if (K <= 0 || K % 256 != 0 || E < 1 || E > gq::kMaxSortExperts || M < 1 || N < 1 || S < 1) return none;
    if (N > gq::kMaxSortPairs || S > gq::kMaxSortPairs || N * S > gq::kMaxSortPairs) return none;
    if (N * S * K * 2 >= ((int64_t)1 << 32)) return none;        // (sgemm_body's 32-bit descriptor over x~)
    const int64_t rb = gq::row_bytes(t, K);
    if (M > INT64_MAX / rb || M * rb >= ((int64_t)1 << 31)) return none; // one expert
    return gq::plan_sgemm_id(E, M, N * S, K);
}

size_t gq_mmq_id_sorted_workspace_size(gq_type t, int64_t E, int64_t M, int64_t N, int64_t S, int64_t K)
{
    if (!gq::known_type(t)) return 0;
    const gq::SortedPlan p = sorted_plan(t, E, M, N, S, K);
    return p.ok ? p.bytes + 15 : 0; // (+15: the entry aligns the workspace to 16 bytes itself)
}

int gq_mmq_id_sorted(gq_type t, const void *A, const int32_t *ids, const void *B, void *C, int64_t E, int64_t M, int64_t N,
                     int64_t S, int64_t K, int64_t ldb, int64_t ldb_slot, int64_t ldc, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    g_err.clear();
    bool empty;
    int rc = check_id_args(t, A, ids, B, C, E, M, N, S, K, ldb, ldb_slot, ldc, empty);
    if (rc != GQ_OK || empty) return rc;
    const gq::SortedPlan p = sorted_plan(t, E, M, N, S, K);
    if (!p.ok)
        return fail(GQ_EUNSUPPORTED,
                    "not a sorted expert GEMM shape (K=%lld %% 256 == 0, E=%lld <= %d, N*S=%lld <= %d, N*S*K*2 < 4 GiB, "
                    "one expert < 2 GiB)",
                    (long long)K, (long long)E, gq::kMaxSortExperts, (long long)(N * S), gq::kMaxSortPairs);
    const size_t need = p.bytes + 15;
    if (!workspace || workspace_bytes < need) return fail_workspace(workspace, workspace_bytes, need);
    uint8_t *ws = (uint8_t *)(((uintptr_t)workspace + 15) & ~(uintptr_t)15);
    uint16_t *xdeq = (uint16_t *)ws;
    int32_t *perm = (int32_t *)(ws + p.perm_off), *hdr = (int32_t *)(ws + p.hdr_off), *table = (int32_t *)(ws + p.table_off);
    const hipStream_t s = (hipStream_t)stream;
    if ((rc = hip_rc(gq::launch_id_sort(ids, N * S, E, p.nb, perm, hdr, table, s), "id sort")) != GQ_OK) return rc;
    rc = hip_rc(gq::launch_act_quant_gather((const uint16_t *)B, ldb, ldb_slot, S, perm, hdr, N * S, K, xdeq, (uint16_t *)C, M,
                                            ldc, s),
                "act gather");
    if (rc != GQ_OK) return rc;
    return hip_rc(gq::launch_sgemm_id(t, (const uint8_t *)A, xdeq, (uint16_t *)C, perm, hdr, table, p, M, K, ldc, s),
                  "sorted GEMM");
}

// gq_mmq_grouped_prepared: the items as the grouped streaming GEMM takes them, or a GQ_* error
// (shape_only: the plan query's items, whose pointers are null and not read)
static int grouped_gemm_items(gq_act act, const gq_gemm_item *items, int n, int64_t N, gq::SGroupItem *out,
                              bool shape_only = false)
{
    if (n < 0 || (n > 0 && !items)) return fail(GQ_EINVAL, "bad item list (n=%d, items=%p)", n, (const void *)items);
    if (n > 16) return fail(GQ_EUNSUPPORTED, "more than 16 items");
    if (N < 5) return fail(GQ_EUNSUPPORTED, "grouped GEMM needs N >= 5 (N=%lld): gq_mmq_grouped for decode", (long long)N);
    for (int i = 0; i < n; ++i) {
        const gq_gemm_item &it = items[i];
        const int rc = check_mmq_shape(it.type, act, it.M, N, it.K);
        if (rc != GQ_OK) return rc;
        if (it.K % 256 != 0 || it.K == 0) return fail(GQ_EUNSUPPORTED, "item %d: K=%lld is not a multiple of 256", i, (long long)it.K);
        if (!shape_only && it.M > 0 && (!it.A || !it.ws || !it.C)) return fail(GQ_EINVAL, "item %d: null pointer", i);
        if (it.ldc < it.M) return fail(GQ_EINVAL, "item %d: ldc=%lld < M=%lld", i, (long long)it.ldc, (long long)it.M);
        if (gq::gemm_rows_per_launch(it.type, it.M, it.K, gq::tuning()) < it.M ||
            gq::gemm_toks_per_launch(N, it.K, gq::tuning()) < N)
            return fail(GQ_EUNSUPPORTED, "item %d: 2 GiB or more in one operand", i);
        out[i] = gq::SGroupItem{it.type, (const uint8_t *)it.A, shape_only ? nullptr : carve(act, const_cast<void *>(it.ws), N, it.K).xdeq,
                                (uint16_t *)it.C, it.ldc, it.M, it.K};
    }
    return GQ_OK;
}

// gq_mmq_grouped_prepared's split of the items: those the K-chunked streaming MMQ takes (one
// launch, no workspace) and the rest (the grouped streaming GEMM: one launch + its reduce).
// The stream's launch holds at most kKMaxParts (item, K range) parts: an item whose ranges would
// pass that goes to the streaming GEMM (e.g. 16 items at K = 8192 are 32 parts: the first 12 take
// the stream, the other 4 the GEMM).
// kid, rid (the plan query): each launch's items as indices of the call's list.
static void grouped_split(gq_act act, gq::SGroupItem *g, int n, int64_t N, gq::KItem *ks, int &nk, gq::SGroupItem *rest,
                          int &nr, int *kid = nullptr, int *rid = nullptr)
{
    nk = nr = 0;
    int parts = 0;
    for (int i = 0; i < n; ++i) {
        if (g[i].M <= 0) continue;
        const int np = gq::kstream_splits(g[i].K);
        if (gq::grouped_kstream_item(g[i].fmt, act, g[i].M, N, g[i].K, g[i].K, g[i].ldc, g[i].C, true, gq::tuning()) &&
            parts + np <= gq::kKMaxParts && (parts += np, true)) {
            if (kid) kid[nk] = i;
            ks[nk++] = gq::KItem{g[i].fmt, g[i].A, g[i].X, g[i].K, g[i].C, g[i].ldc, g[i].M, g[i].K};
        } else {
            if (rid) rid[nr] = i;
            rest[nr++] = g[i];
        }
    }
}

size_t gq_mmq_grouped_prepared_workspace_size(gq_act act, const gq_gemm_item *items, int n, int64_t N)
{
    gq::SGroupItem g[16], rest[16];
    gq::KItem ks[16];
    int nk, nr;
    if (n < 1 || grouped_gemm_items(act, items, n, N, g) != GQ_OK) return 0;
    grouped_split(act, g, n, N, ks, nk, rest, nr);
    // [the K-chunked stream's K-range partials][the streaming GEMM's split-K partials]
    const size_t kb = gq::align_up(gq::kstream_partial_bytes(ks, nk, N));
    if (nr == 0) return kb;
    const gq::SGroupPlan p = gq::plan_sgemm_grouped(rest, nr, N, gq::tuning().sgemm_splits);
    return kb + (p.ok ? p.partial_bytes : 0);
}

int gq_mmq_grouped_prepared(gq_act act, const gq_gemm_item *items, int n, int64_t N, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    g_err.clear();
    gq::SGroupItem g[16], rest[16];
    gq::KItem ks[16];
    int nk, nr;
    int rc = grouped_gemm_items(act, items, n, N, g);
    if (rc != GQ_OK) return rc;
    grouped_split(act, g, n, N, ks, nk, rest, nr);
    // [the K-chunked stream's K-range partials][the streaming GEMM's split-K partials]
    const size_t kb = gq::align_up(gq::kstream_partial_bytes(ks, nk, N));
    gq::SGroupPlan p;
    const size_t need = kb + (nr > 0 ? (p = gq::plan_sgemm_grouped(rest, nr, N, gq::tuning().sgemm_splits)).partial_bytes : 0);
    if (nr > 0 && !p.ok) return fail(GQ_EUNSUPPORTED, "not a grouped GEMM shape");
    if (need && (!workspace || workspace_bytes < need)) return fail_workspace(workspace, workspace_bytes, need);
    if (nk > 0 && (rc = hip_rc(gq::launch_kstream(ks, nk, N, 0, workspace, (hipStream_t)stream), "grouped kstream")) != GQ_OK)
        return rc;
    if (nr > 0)
        return hip_rc(gq::launch_sgemm_grouped(rest, nr, N, p, (uint8_t *)workspace + kb, (hipStream_t)stream), "grouped GEMM");
    return GQ_OK;
}

int gq_mmq_sharded(gq_type t, const void *A_shard, const void *B, void *C, int64_t M, int64_t N, int64_t K,
                   int64_t ldb, int64_t ldc, int world, int rank, void *nccl_comm, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    g_err.clear();
    int rc = check_mmq_shape(t, GQ_ACT_Q8_1, M, N, K);
    if (rc != GQ_OK) return rc;
    if (world < 1 || rank < 0 || rank >= world) return fail(GQ_EINVAL, "bad rank %d of world %d", rank, world);
    if (world > 1 && !nccl_comm) return fail(GQ_EINVAL, "world=%d needs an RCCL communicator", world);
    if (M == 0 || N == 0) return GQ_OK;
    if (K == 0) return fail(GQ_EINVAL, "K must be positive");
    if (!B || !C) return fail(GQ_EINVAL, "null pointer (B=%p C=%p)", B, C);
    if (ldc < M) return fail(GQ_EINVAL, "ldc=%lld < M=%lld", (long long)ldc, (long long)M);
    const size_t need = sharded_ws(t, M, N, K, world);
    if (!workspace || workspace_bytes < need) return fail_workspace(workspace, workspace_bytes, need);
    int64_t row0, rows, R;
    shard_geom(M, world, rank, row0, rows, R);
    if (rows > 0 && !A_shard) return fail(GQ_EINVAL, "null A_shard for %lld rows", (long long)rows);
    uint8_t *ws = (uint8_t *)workspace;
    uint16_t *slab = (uint16_t *)ws;                                      // (N, R)
    uint16_t *gathered = (uint16_t *)(ws + gq::align_up((size_t)N * R * 2)); // (world, N, R)
    uint8_t *mws = (uint8_t *)gathered + gq::align_up((size_t)world * N * R * 2);
    const size_t mws_bytes = workspace_bytes - (size_t)(mws - ws);
    hipStream_t s = (hipStream_t)stream;
    if (rows > 0) {
        rc = gq_mmq(t, A_shard, B, slab, rows, N, K, ldb, R, mws, mws_bytes, stream);
        if (rc != GQ_OK) return rc;
    }
    if (world == 1 && !nccl_comm) // the slab is the output
        return hip_rc(launch_assemble(slab, (uint16_t *)C, N, R, M, ldc, s), "assemble");
    AllGatherFn ag = shard_allgather();
    if (!ag) return fail(GQ_EUNSUPPORTED, "RCCL (ncclAllGather) not found in the process");
    // (a short or empty last shard sends its slab's pad columns too: assemble never reads them)
    const ncclResult_t nr = ag(slab, gathered, (size_t)N * R, ncclFloat16, (ncclComm_t)nccl_comm, s);
    if (nr != ncclSuccess) return fail(GQ_EHIP, "ncclAllGather failed (%d)", (int)nr);
    return hip_rc(launch_assemble(gathered, (uint16_t *)C, N, R, M, ldc, s), "assemble");
}

} // extern "C"

// Each family's entry-point checks ahead of its launcher (gq_mmq_ex's route, gq_mmq_glu's, the id
// entries' pair limits, gq_mmq_grouped_ex's token counts), then the launcher's own plan.
int gq_debug_decode_plan(int family, gq_act act, const gq_group_item *items, int n, int64_t N, gq_decode_plan *out,
                         int max_out)
{
    static_assert(sizeof(gq_decode_plan) == sizeof(gq::DecodePlanInfo), "gq_decode_plan is DecodePlanInfo");
    g_err.clear();
    if (n < 1 || n > 16 || !items || N < 1 || max_out < 0 || (max_out > 0 && !out)) return 0;
    if (family != gq::DF_GROUPED && n != 1) return 0;
    const bool fp8 = act == GQ_ACT_FP8_E4M3;
    gq::DecodeItem di[16];
    for (int i = 0; i < n; ++i) {
        const gq_group_item &it = items[i];
        // (the id families' N is the pair count: no part of the shape checks)
        if (check_mmq_shape(it.type, act, it.M, family == gq::DF_GROUPED ? N : 1, it.K) != GQ_OK || it.M <= 0 || it.K <= 0) {
            g_err.clear();
            return 0;
        }
        di[i] = gq::DecodeItem{it.type, nullptr, nullptr, it.K, nullptr, it.M, it.M, it.K};
    }
    const gq::DecodeItem &d = di[0];
    switch (family) {
    case gq::DF_DENSE:
    case gq::DF_GLU: {
        const gq::Plan p = gq::plan_call(gq::shape_call(d.fmt, act, d.M, N, d.K, false), gq::tuning());
        if (p.kernel != gq::K_DECODE || !p.raw) return 0;
        if (family == gq::DF_GLU && (fp8 || N > gq::kGluMaxTokens)) return 0;
        break;
    }
    case gq::DF_ID:
    case gq::DF_ID_GLU:
        if (fp8 || N > (int64_t)gq::kMaxIdPairs * gq::kMaxIdPairs) return 0;
        break;
    case gq::DF_GROUPED:
        if (N >= (fp8 ? 3 : 5)) return 0; // (the K-chunked stream's token counts)
        break;
    default: return 0;
    }
    return gq::decode_plan_info(family, di, n, N, fp8, (gq::DecodePlanInfo *)out, max_out);
}

// Each entry point's checks and plan ahead of its launches, then the launches as data (plan_entries and
// the kernel files' *_plan_info).
int gq_debug_gemm_plan(int entry, gq_act act, const gq_group_item *items, int n, int64_t N, int64_t E, int64_t S,
                       gq_gemm_plan *out_, int max_out)
{
    static_assert(sizeof(gq_gemm_plan) == sizeof(gq::GemmPlanInfo), "gq_gemm_plan is GemmPlanInfo");
    static_assert((int)GQ_GK_NONE == gq::GK_NONE && (int)GQ_GK_RGEMM == gq::GK_RGEMM && (int)GQ_GK_SGEMM == gq::GK_SGEMM &&
                      (int)GQ_GK_SGEMM_ID == gq::GK_SGEMM_ID && (int)GQ_GK_SGEMM_GROUPED == gq::GK_SGEMM_GROUPED &&
                      (int)GQ_GK_REDUCE_GROUPED == gq::GK_REDUCE_GROUPED && (int)GQ_GK_GEMM == gq::GK_GEMM &&
                      (int)GQ_GK_GEMM_REDUCE_F16 == gq::GK_GEMM_REDUCE_F16 && (int)GQ_GK_GEMM_REDUCE == gq::GK_GEMM_REDUCE &&
                      (int)GQ_GK_SKINNY == gq::GK_SKINNY && (int)GQ_GK_KSTREAM == gq::GK_KSTREAM &&
                      (int)GQ_GK_KSTREAM_REDUCE == gq::GK_KSTREAM_REDUCE,
                  "GQ_GK_* is GemmKernelId");
    g_err.clear();
    gq::GemmPlanInfo *out = (gq::GemmPlanInfo *)out_;
    if (n < 1 || n > 16 || !items || N < 1 || max_out < 0 || (max_out > 0 && !out)) return 0;
    if (entry >= 0 && entry <= 2 && n != 1) return 0;
    const gq_group_item &d = items[0];
    int cnt = 0;
    switch (entry) {
    case 0:   // gq_mmq_ex
    case 1: { // gq_mmq_prepared_ex
        if (check_mmq_shape(d.type, act, d.M, N, d.K) != GQ_OK || d.M <= 0 || d.K <= 0) break;
        gq::Call c = gq::shape_call(d.type, act, d.M, N, d.K, entry == 1);
        gq::Plan p = gq::plan_call(c, gq::tuning());
        if (entry == 0 && !runs_own_plan(p)) { // (act_quant, then run_prepared)
            c = gq::shape_call(d.type, act, d.M, N, d.K, true);
            p = gq::plan_call(c, gq::tuning());
        }
        cnt = plan_entries(c, p, out, 0, max_out);
        break;
    }
    case 2: { // gq_mmq_id_sorted: N tokens x S slots on E experts
        if (!gq::known_type(d.type) || d.M <= 0 || d.K <= 0) break;
        cnt = gq::sgemm_id_plan_info(d.type, sorted_plan(d.type, E, d.M, N, S, d.K), d.M, d.K, out, 0, max_out);
        break;
    }
    case 3: { // gq_mmq_grouped_prepared
        gq_gemm_item gi[16];
        gq::SGroupItem g[16], rest[16];
        gq::KItem ks[16];
        int nk, nr, kid[16], rid[16];
        for (int i = 0; i < n; ++i) gi[i] = gq_gemm_item{items[i].type, nullptr, nullptr, nullptr, items[i].M, items[i].M, items[i].K};
        if (grouped_gemm_items(act, gi, n, N, g, true) != GQ_OK) break;
        grouped_split(act, g, n, N, ks, nk, rest, nr, kid, rid);
        gq::SGroupPlan p;
        if (nr > 0 && !(p = gq::plan_sgemm_grouped(rest, nr, N, gq::tuning().sgemm_splits)).ok) break; // (refused)
        if (nk > 0) cnt = gq::kstream_plan_info(ks, nk, N, 0, kid, out, cnt, max_out);
        if (nr > 0) cnt = gq::sgemm_grouped_plan_info(rest, nr, N, p, rid, out, cnt, max_out);
        break;
    }
    case 4: { // gq_mmq_grouped_ex on the K-chunked stream
        if (!grouped_ex_is_kstream(act, N)) break;
        gq::KItem ki[16];
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const gq_group_item &it = items[i];
            if (check_mmq_shape(it.type, act, it.M, N, it.K) != GQ_OK || it.K <= 0) return g_err.clear(), 0;
            if (it.M == 0) continue;
            const gq::DecodeItem di{it.type, nullptr, nullptr, it.K, nullptr, it.M, it.M, it.K};
            if (!grouped_ex_kstream_item(di, act, N)) return 0;
            ki[m++] = gq::KItem{di.fmt, di.A, di.X, di.ldx, di.C, di.ldc, di.M, di.K};
        }
        if (m > 0) cnt = gq::kstream_plan_info(ki, m, N, act == GQ_ACT_FP8_E4M3 ? 2 : 1, nullptr, out, 0, max_out);
        break;
    }
    default: break;
    }
    g_err.clear();
    return cnt;
}

int gq_debug_decode_cap(int family, int set, gq_type t, int nt, int fp8)
{
    return gq::decode_itc_cap(family, set, t, nt, fp8 != 0);
}

const char *gq_debug_route(gq_type t, gq_act act, int64_t M, int64_t N, int64_t K, int prepared)
{
    if (check_mmq_shape(t, act, M, N, K) != GQ_OK || M <= 0 || N <= 0 || K <= 0) return "none";
    g_err.clear();
    const gq::Call c = gq::shape_call(t, act, M, N, K, prepared != 0);
    return gq::route_name(c, gq::plan_call(c, gq::tuning()));
}

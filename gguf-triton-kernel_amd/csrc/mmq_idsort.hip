// mmq_idsort.hip -- the device-side sort of the sorted expert GEMM (gq_mmq_id_sorted): the
// router's (token, slot) pairs grouped by expert, with the token-tile table the GEMM launch
// (mmq_rgemm.hip sgemm_id_kernel) walks.  What a host that had read the ids would hand the
// streaming GEMM, made on the device instead: no host sync, one launch whose grid does not
// depend on the ids.
//
// One workgroup of 16 waves, a stable counting sort:
//   1. wave w counts the buckets of ITS contiguous range of pairs into its own LDS histogram
//      (bucket = the expert, or E for an id outside [0, E));
//   2. the buckets' totals are scanned (exclusive): base[b] = first sorted row of bucket b, and
//      the per-expert tile counts ceil(cnt / BN) likewise: ts[e] = expert e's first table entry;
//   3. wave w's histogram becomes its cursors: base[b] + the counts of the waves before it;
//   4. wave w walks its range in order, 64 pairs at a time; the lanes that share a bucket take
//      consecutive places by lane (ballot + popcount), so a bucket's pairs end up in ascending
//      pair index whatever the timing: the permutation is a function of the ids alone;
//   5. table entry i = (expert, first sorted row, rows <= BN), found by bisecting ts.
// Out-of-range pairs sort last (rows [nvalid, P)); no table entry covers them -- the gather
// launch zeroes their outputs.  Everything leaves through ordinary vector stores.
#include "gguf_internal.hpp"

namespace gq {

namespace {

constexpr int SORT_WAVES = 16, SORT_THREADS = 64 * SORT_WAVES;
constexpr int SORT_NBK = kMaxSortExperts + 1; // buckets at most

// exclusive scan over the workgroup of two values per thread (elements 2*tid, 2*tid + 1 of a
// sequence); returns the total.  wsum: SORT_WAVES ints of LDS.
__device__ __forceinline__ int block_scan2(int a0, int a1, int *wsum, int &e0, int &e1)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = a0 + a1;
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < SORT_WAVES; ++w) {
        const int v = wsum[w];
        if (w < wave) before += v;
        total += v;
    }
    __syncthreads(); // (wsum may be reused)
    e0 = before + incl - s;
    e1 = e0 + a0;
    return total;
}

__global__ __launch_bounds__(SORT_THREADS) void id_sort_kernel(const int32_t *__restrict__ ids, int P, int E, int BN,
                                                               int32_t *__restrict__ perm, int32_t *__restrict__ hdr,
                                                               int32_t *__restrict__ table)
{
    __shared__ int cur[SORT_WAVES * SORT_NBK]; // [wave][bucket], row stride nbk
    __shared__ int cnt[2 * SORT_THREADS], base[2 * SORT_THREADS], ts[2 * SORT_THREADS];
    __shared__ int wsum[SORT_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nbk = E + 1;
    auto bucket = [E](int id) { return (unsigned)id < (unsigned)E ? id : E; };

    for (int i = tid; i < SORT_WAVES * nbk; i += SORT_THREADS) cur[i] = 0;
    __syncthreads();
    // 1. per-wave histograms of contiguous ranges (whole 64-pair steps)
    const int chunk = ((P + SORT_WAVES - 1) / SORT_WAVES + 63) & ~63;
    const int lo = wave * chunk < P ? wave * chunk : P, hi = lo + chunk < P ? lo + chunk : P;
    int *mine = cur + wave * nbk;
    for (int i = lo + lane; i < hi; i += 64) atomicAdd(&mine[bucket(ids[i])], 1);
    __syncthreads();
    // 2. totals, their scan, the tile counts' scan
    for (int b = tid; b < 2 * SORT_THREADS; b += SORT_THREADS) {
        int t = 0;
        if (b < nbk)
            for (int w = 0; w < SORT_WAVES; ++w) t += cur[w * nbk + b];
        cnt[b] = t;
    }
    __syncthreads();
    const int c0 = cnt[2 * tid], c1 = cnt[2 * tid + 1];
    int e0, e1;
    block_scan2(c0, c1, wsum, e0, e1);
    base[2 * tid] = e0;
    base[2 * tid + 1] = e1;
    const int n0 = 2 * tid < E ? (c0 + BN - 1) / BN : 0, n1 = 2 * tid + 1 < E ? (c1 + BN - 1) / BN : 0;
    const int T = block_scan2(n0, n1, wsum, e0, e1);
    ts[2 * tid] = e0;     // (ts[e] for e >= E: T)
    ts[2 * tid + 1] = e1;
    __syncthreads();
    // 3. histograms -> cursors
    for (int b = tid; b < nbk; b += SORT_THREADS) {
        int run = base[b];
        for (int w = 0; w < SORT_WAVES; ++w) {
            const int c = cur[w * nbk + b];
            cur[w * nbk + b] = run;
            run += c;
        }
    }
    __syncthreads();
    // 4. the stable scatter
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool live = i < hi;
        const int b = live ? bucket(ids[i]) : -1;
        unsigned long long todo = __ballot(live);
        while (todo) {
            const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            const int v = __builtin_amdgcn_readlane(b, leader);
            const unsigned long long m = __ballot(b == v);
            const int start = mine[v]; // (every lane: the same word, read before the leader's update)
            if (b == v) perm[start + __popcll(m & ((1ull << lane) - 1))] = i;
            if (lane == leader) mine[v] = start + __popcll(m);
            todo &= ~m;
        }
    }
    // 5. the tile table
    for (int i = tid; i < T; i += SORT_THREADS) {
        int a = 0, z = E; // the last e in [0, E) with ts[e] <= i (then ts[e + 1] > i: e has rows)
        while (z - a > 1) {
            const int mid = (a + z) >> 1;
            if (ts[mid] <= i) a = mid;
            else z = mid;
        }
        const int j = i - ts[a], left = cnt[a] - j * BN;
        table[4 * i + 0] = a;
        table[4 * i + 1] = base[a] + j * BN;
        table[4 * i + 2] = left < BN ? left : BN;
        table[4 * i + 3] = 0;
    }
    if (tid == 0) {
        hdr[0] = T;
        hdr[1] = base[E]; // nvalid: the out-of-range pairs are sorted rows [nvalid, P)
        hdr[2] = 0;
        hdr[3] = 0;
    }
}

} // namespace

hipError_t launch_id_sort(const int32_t *ids, int64_t P, int64_t E, int nb, int32_t *perm, int32_t *hdr, int32_t *table,
                          hipStream_t s)
{
    if (P < 1 || P > kMaxSortPairs || E < 1 || E > kMaxSortExperts || nb < 1) return hipErrorInvalidValue;
    id_sort_kernel<<<dim3(1), dim3(SORT_THREADS), 0, s>>>(ids, (int)P, (int)E, 16 * nb, perm, hdr, table);
    return hipGetLastError();
}

} // namespace gq

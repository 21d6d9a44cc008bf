// arl_cooccur.hip -- exact top-k co-occurrence neighbours of the rows of a sparse binary matrix on gfx950 (no reference counterpart: the
// primitive under the classical profile detectors, DegSim and kNN in-degree, and under an item-kNN neighbour list on the transposed input).
//
// X is n_rows x n_cols, binary, given as CSR plus its column-major index (rows ascending within a column).  For a query row u the kernel lists
// up to k other rows v with c(u, v) = |X_u & X_v| > 0, best first by the measure (count, cosine, Jaccard), ties to the smaller row id.  The
// n_rows x n_rows product is never formed.  A workgroup owns one query.  Its LDS holds int32 counters for a tile of candidate rows, the sorted
// list of the k best so far, and a pending buffer.  Per tile it clears the counters, walks the query's columns (waves over columns, lanes over
// the column's rows inside the tile, ds_add on the counter), then scans the counters: a nonzero v != u that beats the current k-th entry goes
// to the pending buffer, and when that would overflow the list and the buffer are merged by ranking (every element counts the elements that
// beat it; rank < k is its place in the new list).
//
// Rules kept:
//   * the order is decided in integers only.  For a fixed u cosine compares c1^2 d2 with c2^2 d1 and Jaccard c1 (du + d2 - c2) with
//     c2 (du + d1 - c1), in 64 bits: exact while every degree is <= 2^20 (cosine; arl_cooccur_max_degree) or < 2^31 (count, Jaccard).  With the
//     id as tie-break the order is strict and total, so the result is a function of the input alone: the same bits from run to run, whatever
//     order the LDS atomics and the pending slots take;
//   * where a tile starts inside a column is known without a search while the query has at most kCur columns (a cursor per column in LDS,
//     advanced tile by tile because rows ascend), and found by binary search past that;
//   * counters are 32-bit; no global atomics, no float atomics, no workspace: the only global writes are the query's 2k output words, each
//     written exactly once (the padding idx = -1, cnt = 0 included, also for an empty or out-of-range query);
//   * ids outside [0, n_rows) / [0, n_cols) are skipped, never turned into an address; rowptr and colptr are trusted.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "arlib_amd.h"

namespace {

constexpr int kBlk = 256, kWaves = kBlk / 64;
constexpr int kMaxK = 128;                                      // the list
constexpr int kPend = 1024;                                     // the pending buffer
constexpr int kEnt = kMaxK + kPend;
constexpr int kPer = (kEnt + kBlk - 1) / kBlk;                  // elements a thread ranks in a merge
constexpr int kCur = 512;                                       // column cursors
constexpr int kHead = 16;                                       // header words: list length, pending length, candidate count
constexpr int kFixedWords = kHead + kCur + 3 * kEnt;            // 3 984 words = 15 936 bytes, a multiple of 16
constexpr int64_t kLdsBytes = 160 * 1024;                       // LDS of one CU of gfx950
constexpr int kMaxTile = 36864;                                 // 15 936 + 4 * 36 864 = 163 392 <= 163 840
constexpr int kDefaultTile = 16384;                             // 15 936 + 65 536 = 81 472 <= 80 KiB: two workgroups per CU
constexpr int64_t kMaxDegreeCosine = 1ll << 20;                 // c^2 d <= 2^60
enum { LIST_N = 0, PEND_N = 1, CAND = 2 };
static_assert(kFixedWords % 4 == 0 && (int64_t)kFixedWords * 4 + (int64_t)kMaxTile * 4 <= kLdsBytes, "LDS budget");
static_assert((int64_t)kFixedWords * 4 + (int64_t)kDefaultTile * 4 <= kLdsBytes / 2, "two workgroups per CU at the default tile");

// a = (ca, da, ia) comes before b in the list of a query of degree du
template <int M>
__device__ __forceinline__ bool beats(int ca, int da, int ia, int cb, int db, int ib, int du) {
    uint64_t ka, kb;
    if (M == 0) {
        ka = (uint64_t)ca;
        kb = (uint64_t)cb;
    } else if (M == 1) {
        ka = (uint64_t)ca * (uint64_t)ca * (uint64_t)db;
        kb = (uint64_t)cb * (uint64_t)cb * (uint64_t)da;
    } else {
        ka = (uint64_t)ca * (uint64_t)((int64_t)du + db - cb);
        kb = (uint64_t)cb * (uint64_t)((int64_t)du + da - ca);
    }
    return ka > kb || (ka == kb && ia < ib);
}

// list [0, ln) and pending [kMaxK, kMaxK + pn) -> the min(ln + pn, K) best, sorted, in [0, ..).  Called by the whole workgroup after a barrier
// behind the last append; ends with a barrier.
template <int M>
__device__ void merge(int *hdr, int *ec, int *ed, int *ei, int K, int du) {
    const int tid = threadIdx.x;
    const int ln = hdr[LIST_N], pn = min(hdr[PEND_N], kPend), n = ln + pn;
    int mc[kPer], md[kPer], mi[kPer], mr[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = tid + j * kBlk;
        mr[j] = INT_MAX;
        if (e < n) {
            const int s = e < ln ? e : kMaxK + (e - ln);
            mc[j] = ec[s], md[j] = ed[s], mi[j] = ei[s];
            int r = 0;
            for (int f = 0; f < ln; ++f) r += beats<M>(ec[f], ed[f], ei[f], mc[j], md[j], mi[j], du) ? 1 : 0;
            for (int f = kMaxK; f < kMaxK + pn; ++f) r += beats<M>(ec[f], ed[f], ei[f], mc[j], md[j], mi[j], du) ? 1 : 0;
            mr[j] = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        if (mr[j] < K) ec[mr[j]] = mc[j], ed[mr[j]] = md[j], ei[mr[j]] = mi[j];
    if (tid == 0) hdr[LIST_N] = min(n, K), hdr[PEND_N] = 0;
    __syncthreads();
}

template <int M>
__global__ __launch_bounds__(kBlk) void cooccur_topk_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                             const int64_t *__restrict__ colptr, const int32_t *__restrict__ irow,
                                                             const int32_t *__restrict__ rows, const int32_t *__restrict__ order, int n_rows,
                                                             int n_cols, int n_q, int K, int T, int32_t *__restrict__ idx,
                                                             int32_t *__restrict__ cnt) {
    extern __shared__ __attribute__((aligned(16))) int lds[];
    int *hdr = lds, *cur = lds + kHead, *ec = cur + kCur, *ed = ec + kEnt, *ei = ed + kEnt, *ctr = ei + kEnt;
    const int slot = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)slot >= (unsigned)n_q) return;                // `order` is a permutation of the slots; anything else is dropped
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t *oi = idx + (int64_t)slot * K, *oc = cnt + (int64_t)slot * K;
    const int u = rows ? rows[slot] : slot;
    int64_t ub = 0, ue = 0;
    if ((unsigned)u < (unsigned)n_rows) ub = rowptr[u], ue = rowptr[u + 1];
    if (ue <= ub) {                                             // uniform over the workgroup: no barrier is skipped by part of it
        for (int j = tid; j < K; j += kBlk) oi[j] = -1, oc[j] = 0;
        return;
    }
    const int du = (int)(ue - ub);
    const bool use_cur = du <= kCur;
    if (tid == 0) hdr[LIST_N] = 0, hdr[PEND_N] = 0, hdr[CAND] = 0;

    for (int t0 = 0; t0 < n_rows; t0 += T) {
        const int t1 = min(t0 + T, n_rows), tl = t1 - t0;
        __syncthreads();                                        // the previous tile's scan is over
        for (int i = tid; i < tl; i += kBlk) ctr[i] = 0;
        __syncthreads();
        for (int64_t p = ub + wv; p < ue; p += kWaves) {
            const int c = col[p];
            if ((unsigned)c >= (unsigned)n_cols) continue;
            const int64_t cb = colptr[c], ce = colptr[c + 1];
            const int j = (int)(p - ub);
            int64_t start = cb;
            if (t0 > 0) {
                if (use_cur) {
                    start = cb + cur[j];
                } else {
                    int64_t lo = cb, hi = ce;
                    while (lo < hi) {
                        const int64_t mid = (lo + hi) >> 1;
                        if (irow[mid] < t0) lo = mid + 1; else hi = mid;
                    }
                    start = lo;
                }
            }
            for (;;) {
                const int64_t q = start + lane;
                const int r = q < ce ? irow[q] : INT_MAX;
                if ((unsigned)(r - t0) < (unsigned)tl) atomicAdd(&ctr[r - t0], 1);
                const int n = __popcll(__ballot(r < t1));
                start += n;
                if (n < 64) break;
            }
            if (use_cur && lane == 0) cur[j] = (int)(start - cb);
        }
        __syncthreads();

        // the counters hold c(u, v) for the tile's rows.  Count what would be appended, then append where it fits.
        int tc = 0, td = 1, ti = INT_MAX;
        bool has_thr = hdr[LIST_N] == K;
        if (has_thr) tc = ec[K - 1], td = ed[K - 1], ti = ei[K - 1];
        int n = 0;
        for (int i = tid; i < tl; i += kBlk) {
            const int c = ctr[i], v = t0 + i;
            if (c > 0 && v != u) n += (!has_thr || beats<M>(c, (int)(rowptr[v + 1] - rowptr[v]), v, tc, td, ti, du)) ? 1 : 0;
        }
        if (n) atomicAdd(&hdr[CAND], n);
        __syncthreads();
        const int cand = hdr[CAND], pn = hdr[PEND_N];
        __syncthreads();
        if (tid == 0) hdr[CAND] = 0;
        if (cand == 0) continue;
        // One piece when the tile's candidates fit the buffer; else pieces, merged after each.  While the list is not full there is no k-th entry
        // to refuse a candidate, so pieces are short (kBlk rows) and pending entries are merged at once: a merge costs the square of what it
        // ranks, and the first one gives every later row a bound to fail against.
        bool whole = cand <= (has_thr ? kPend : kBlk);
        if (pn > 0 && (!whole || !has_thr || pn + cand > kPend)) {
            merge<M>(hdr, ec, ed, ei, K, du);
            has_thr = hdr[LIST_N] == K;
            if (has_thr) tc = ec[K - 1], td = ed[K - 1], ti = ei[K - 1];
            whole = cand <= (has_thr ? kPend : kBlk);
        }
        for (int base = 0; base < tl;) {                        // pieces start with an empty buffer; a whole tile with pn + cand <= kPend
            const int end = whole ? tl : min(base + (has_thr ? kPend : kBlk), tl);
            for (int i = base + tid; i < end; i += kBlk) {
                const int c = ctr[i], v = t0 + i;
                if (c <= 0 || v == u) continue;
                const int d = (int)(rowptr[v + 1] - rowptr[v]);
                if (has_thr && !beats<M>(c, d, v, tc, td, ti, du)) continue;
                const int s = atomicAdd(&hdr[PEND_N], 1);
                if (s < kPend) ec[kMaxK + s] = c, ed[kMaxK + s] = d, ei[kMaxK + s] = v;
            }
            if (!whole) {
                __syncthreads();
                merge<M>(hdr, ec, ed, ei, K, du);
                has_thr = hdr[LIST_N] == K;
                if (has_thr) tc = ec[K - 1], td = ed[K - 1], ti = ei[K - 1];
            }
            base = end;
        }
    }
    __syncthreads();
    if (hdr[PEND_N] > 0) merge<M>(hdr, ec, ed, ei, K, du);       // uniform: nobody writes the word before the merge's first barrier
    const int ln = hdr[LIST_N];
    for (int j = tid; j < K; j += kBlk) oi[j] = j < ln ? ei[j] : -1, oc[j] = j < ln ? ec[j] : 0;
}

}  // namespace

extern "C" {

int64_t arl_cooccur_max_k(void) { return kMaxK; }
int64_t arl_cooccur_max_tile_rows(void) { return kMaxTile; }
int64_t arl_cooccur_default_tile_rows(void) { return kDefaultTile; }
int64_t arl_cooccur_max_degree(int32_t measure) { return measure == ARL_COOCCUR_COSINE ? kMaxDegreeCosine : 0x7fffffffll; }

int arl_cooccur_topk_i32(const int64_t *rowptr, const int32_t *col, const int64_t *colptr, const int32_t *irow, int64_t n_rows, int64_t n_cols,
                         const int32_t *rows, int64_t n_queries, int64_t k, int32_t measure, int64_t max_degree, const int32_t *order,
                         int64_t tile_rows, int32_t *idx, int32_t *cnt, arl_stream_t stream) {
    if (n_rows < 0 || n_cols < 0 || n_queries < 0 || k < 1 || tile_rows < 0 || max_degree < 0) return ARL_E_ARG;
    if (measure != ARL_COOCCUR_COUNT && measure != ARL_COOCCUR_COSINE && measure != ARL_COOCCUR_JACCARD) return ARL_E_ARG;
    if (k > kMaxK || tile_rows > kMaxTile || n_rows > 0x7fffffffll || n_cols > 0x7fffffffll || n_queries > 0x7fffffffll) return ARL_E_RANGE;
    if (n_queries * k > 0x7fffffffll || max_degree > arl_cooccur_max_degree(measure)) return ARL_E_RANGE;
    if (n_queries == 0) return ARL_OK;
    if (!rowptr || !colptr || !idx || !cnt) return ARL_E_NULL;  // col / irow may be NULL for a matrix without entries
    int64_t T = tile_rows ? tile_rows : kDefaultTile;
    if (T > n_rows) T = n_rows > 0 ? n_rows : 1;
    const size_t shm = sizeof(int) * (size_t)(kFixedWords + T);
    const void *fn = measure == ARL_COOCCUR_COUNT    ? (const void *)cooccur_topk_kernel<0>
                     : measure == ARL_COOCCUR_COSINE ? (const void *)cooccur_topk_kernel<1>
                                                     : (const void *)cooccur_topk_kernel<2>;
    if (shm > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)n_queries), block(kBlk);
    const hipStream_t s = (hipStream_t)stream;
    const int nr = (int)n_rows, nc = (int)n_cols, nq = (int)n_queries, K = (int)k, Ti = (int)T;
    if (measure == ARL_COOCCUR_COUNT)
        hipLaunchKernelGGL(cooccur_topk_kernel<0>, grid, block, shm, s, rowptr, col, colptr, irow, rows, order, nr, nc, nq, K, Ti, idx, cnt);
    else if (measure == ARL_COOCCUR_COSINE)
        hipLaunchKernelGGL(cooccur_topk_kernel<1>, grid, block, shm, s, rowptr, col, colptr, irow, rows, order, nr, nc, nq, K, Ti, idx, cnt);
    else
        hipLaunchKernelGGL(cooccur_topk_kernel<2>, grid, block, shm, s, rowptr, col, colptr, irow, rows, order, nr, nc, nq, K, Ti, idx, cnt);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : ARL_OK;
}

}  // extern "C"

// arl_itemknn.hip -- exact fixed-point item-kNN scoring and full-catalogue top-N on gfx950 (no reference counterpart: the scoring step of an
// item-based neighbourhood recommender, arlib_amd/recommender/ItemKNN.py, on the neighbour lists arl_cooccur.hip writes for the transposed input).
//
// X is the binary n_users x n_items matrix as CSR (columns ascending and distinct within a row).  Item j lists k neighbours nbr_idx[j, r] with
// non-negative 32-bit weights nbr_w[j, r]; a slot with nbr_idx < 0 is unused.  The score of item i for user u is
//     s(u, i) = sum over j in P_u, r < k of [nbr_idx[j, r] == i] nbr_w[j, r],
// exact in 64 bits whatever the order of summation.  Every item of the catalogue is a candidate, score 0 included (with mask_profile the items
// of P_u are not); the order is (score descending, item id ascending), strict and total, so the result is a function of the input alone.  The
// n_users x n_items product is never formed.  A workgroup owns one query.  Its LDS holds 64-bit accumulators for a tile of items, the sorted
// list of the N best so far, a pending buffer and the targets' counters.  Per tile it clears the accumulators, walks the profile (waves over
// profile items, lanes over the k slots, a 64-bit ds add on the accumulator of every entry that falls in the tile), marks the profile's own
// items as excluded (the profile is sorted: one contiguous range), then scans the accumulators: a candidate that beats the worst live target
// finds by bisection the first target it beats and adds one to that position's counter, and a candidate that beats the current N-th entry goes
// to the pending buffer, merged by ranking as in arl_cooccur.hip (a copy of that merge on (int64 score, id) entries: the entries differ in
// type and the comparison in arity, and arl_cooccur.hip stays as it is).
//
// Rules kept:
//   * the targets' own scores come from a first pass over the profile, before the first tile: every entry bisects the id-sorted target list
//     and adds its weight to the target it names; the live targets are then sorted best first, so "beats target p" is monotone in p and a
//     candidate adds to one counter; rank[t] is the prefix sum of the counters up to t's position.  A target the mask excludes gets rank -1;
//   * accumulators and target scores are 64-bit LDS integers; no global atomics, no float atomics, no workspace: the only global writes are the
//     query's 2N list words and T rank words, each written exactly once (the padding idx = -1, score = 0 included, also for an empty profile,
//     a profile holding the whole catalogue or a query id outside [0, n_users));
//   * neighbour ids outside [0, n_items) never match a tile or a target and so never become an address; rowptr and col are trusted.
//
// The user side (arlib_amd/userknn.py, recommender/UserKNN.py) is the same kernel with another filling of the accumulators
// and the target scores; the side is a template parameter, the selection is shared.  There user u lists k neighbour users nbr_idx[u, r] with
// weights nbr_w[u, r], and
//     s(u, i) = sum over r < k with v = nbr_idx[u, r] in [0, n_users) of nbr_w[u, r] [i in P_v].
// A cursor, an end and the weight per slot live in LDS.  Per tile [t0, t1) waves go over the slots and lanes over the neighbour's row from its
// cursor: the row is sorted, so its entries below t1 are a prefix, every one gets the slot's weight added to its accumulator, and the cursor
// moves on by the ballot's count until a chunk reaches t1 or the row's end.  Every entry of a neighbour's row is read once, plus at most one
// re-read chunk per tile seam.  The targets' scores come from one bisection per (slot, target) pair in the neighbour's row.  A neighbour id
// outside [0, n_users) leaves its slot empty and never becomes an address.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include "arlib_amd.h"

namespace {

constexpr int kBlk = 256, kWaves = kBlk / 64;
constexpr int kMaxN = 128;                                      // the list
constexpr int kMaxK = 128;                                      // neighbour slots per item
constexpr int kMaxT = 64;                                       // targets
constexpr int kPend = 1024;                                     // the pending buffer
constexpr int kEnt = kMaxN + kPend;
constexpr int kPer = (kEnt + kBlk - 1) / kBlk;                  // elements a thread ranks in a merge
constexpr int kHead = 16;                                       // header words: list length, pending length, candidate count, live targets
constexpr int kHist = kMaxT + 16;                               // one counter per sorted target position
// bytes: entry scores, entry ids, target scores (by id), sorted target scores, then five int[kMaxT] (ids by id, columns by id, live flags,
// sorted ids, sorted columns), the counters, the header
constexpr int kFixedBytes = 8 * kEnt + 4 * kEnt + 8 * kMaxT + 8 * kMaxT + 5 * 4 * kMaxT + 4 * kHist + 4 * kHead;    // 16 512
constexpr int64_t kLdsBytes = 160 * 1024;                       // LDS of one CU of gfx950
constexpr int kMaxTile = 18400;                                 // 16 512 + 8 * 18 400 = 163 712 <= 163 840
constexpr int kDefaultTile = 8160;                              // 16 512 + 8 * 8 160 = 81 792 <= 80 KiB: two workgroups per CU
enum { LIST_N = 0, PEND_N = 1, CAND = 2, LIVE_T = 3 };
static_assert(kFixedBytes % 16 == 0 && (int64_t)kFixedBytes + 8ll * kMaxTile <= kLdsBytes, "LDS budget");
static_assert((int64_t)kFixedBytes + 8ll * kDefaultTile <= kLdsBytes / 2, "two workgroups per CU at the default tile");
// the user side adds a cursor and an end (64-bit) and a weight per neighbour slot
constexpr int kUserFixedBytes = kFixedBytes + (8 + 8 + 4) * kMaxK;                                                  // 19 072
constexpr int kUserMaxTile = 18096;                             // 19 072 + 8 * 18 096 = 163 840
constexpr int kUserDefaultTile = 7856;                          // 19 072 + 8 * 7 856 = 81 920 = 80 KiB: two workgroups per CU
static_assert(kUserFixedBytes % 16 == 0 && (int64_t)kUserFixedBytes + 8ll * kUserMaxTile <= kLdsBytes, "LDS budget, user side");
static_assert((int64_t)kUserFixedBytes + 8ll * kUserDefaultTile <= kLdsBytes / 2, "two workgroups per CU at the default tile, user side");

// a = (sa, ia) comes before b: the larger score, then the smaller id
__device__ __forceinline__ bool beats(int64_t sa, int ia, int64_t sb, int ib) { return sa > sb || (sa == sb && ia < ib); }

// list [0, ln) and pending [kMaxN, kMaxN + pn) -> the min(ln + pn, N) best, sorted, in [0, ..).  Called by the whole workgroup after a barrier
// behind the last append; ends with a barrier.  (arl_cooccur.hip's merge, on (score, id) entries.)
__device__ void merge(int *hdr, int64_t *es, int *ei, int N) {
    const int tid = threadIdx.x;
    const int ln = hdr[LIST_N], pn = min(hdr[PEND_N], kPend), n = ln + pn;
    int64_t ms[kPer];
    int mi[kPer], mr[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int e = tid + j * kBlk;
        mr[j] = INT_MAX;
        if (e < n) {
            const int s = e < ln ? e : kMaxN + (e - ln);
            ms[j] = es[s], mi[j] = ei[s];
            int r = 0;
            for (int f = 0; f < ln; ++f) r += beats(es[f], ei[f], ms[j], mi[j]) ? 1 : 0;
            for (int f = kMaxN; f < kMaxN + pn; ++f) r += beats(es[f], ei[f], ms[j], mi[j]) ? 1 : 0;
            mr[j] = r;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kPer; ++j)
        if (mr[j] < N) es[mr[j]] = ms[j], ei[mr[j]] = mi[j];
    if (tid == 0) hdr[LIST_N] = min(n, N), hdr[PEND_N] = 0;
    __syncthreads();
}

// first position in [0, n) of the ascending list a whose value is >= x
__device__ __forceinline__ int lower_bound_lds(const int *a, int n, int x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// kUser = false: the item side, lists indexed by item.  kUser = true: the user side, lists indexed by user.  The two instances differ in how the
// accumulators and the target scores are filled and in nothing else.
template <bool kUser>
__global__ __launch_bounds__(kBlk) void knn_score_topk_kernel(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                               const int32_t *__restrict__ nbr_idx, const int32_t *__restrict__ nbr_w,
                                                               const int32_t *__restrict__ rows, const int32_t *__restrict__ order,
                                                               const int32_t *__restrict__ tgt_id, const int32_t *__restrict__ tgt_col,
                                                               int n_users, int n_items, int n_q, int K, int N, int NT, int mask_profile,
                                                               int T, int32_t *__restrict__ idx, int64_t *__restrict__ score,
                                                               int32_t *__restrict__ rank) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    int64_t *es = (int64_t *)lds, *tsc = es + kEnt, *ss = tsc + kMaxT;
    int *ei = (int *)(ss + kMaxT), *tgi = ei + kEnt, *tgc = tgi + kMaxT, *tlive = tgc + kMaxT, *si = tlive + kMaxT, *sc = si + kMaxT;
    int *hist = sc + kMaxT, *hdr = hist + kHist;
    int64_t *acc = (int64_t *)(lds + (kUser ? kUserFixedBytes : kFixedBytes));
    int64_t *cur = (int64_t *)(lds + kFixedBytes), *cend = cur + kMaxK;     // user side only: the slots' cursors, ends and weights
    uint32_t *cw = (uint32_t *)(cend + kMaxK);
    const int slot = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)slot >= (unsigned)n_q) return;                // `order` is a permutation of the slots; anything else is dropped
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int32_t *oi = idx + (int64_t)slot * N;
    int64_t *os = score + (int64_t)slot * N;
    const int u = rows ? rows[slot] : slot;
    int64_t ub = 0, ue = 0;
    if ((unsigned)u < (unsigned)n_users) ub = rowptr[u], ue = rowptr[u + 1];
    if (ue < ub) ue = ub;
    if (tid == 0) hdr[LIST_N] = 0, hdr[PEND_N] = 0, hdr[CAND] = 0, hdr[LIVE_T] = 0;
    for (int j = tid; j < kHist; j += kBlk) hist[j] = 0;
    if constexpr (kUser) {                                      // a slot without a neighbour in [0, n_users) is an empty row
        if (tid < K) {
            const int v = (unsigned)u < (unsigned)n_users ? nbr_idx[(int64_t)u * K + tid] : -1;
            int64_t b = 0, e = 0;
            uint32_t w = 0;
            if ((unsigned)v < (unsigned)n_users) b = rowptr[v], e = rowptr[v + 1], w = (uint32_t)nbr_w[(int64_t)u * K + tid];
            cur[tid] = b, cend[tid] = e < b ? b : e, cw[tid] = w;
        }
    }

    // ---- the targets: their scores from a first pass over the profile, then the live ones sorted best first
    int nlive = 0;
    if (NT > 0) {                                               // uniform over the workgroup
        if (tid < NT) tgi[tid] = tgt_id[tid], tgc[tid] = tgt_col[tid], tsc[tid] = 0;
        __syncthreads();
        if constexpr (kUser) {                                  // every (slot, target) pair bisects the target in the neighbour's row
            for (int pr = tid; pr < K * NT; pr += kBlk) {
                const int r = pr / NT, t = pr - r * NT;
                const int x = tgi[t];
                int64_t lo = cur[r];
                const int64_t e = cend[r];
                int64_t hi = e;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (col[mid] < x) lo = mid + 1; else hi = mid;
                }
                if (lo < e && col[lo] == x) atomicAdd((unsigned long long *)&tsc[t], (unsigned long long)cw[r]);
            }
        } else {
            for (int64_t p = ub + wv; p < ue; p += kWaves) {
                const int j = col[p];
                if ((unsigned)j >= (unsigned)n_items) continue;
                for (int r = lane; r < K; r += 64) {
                    const int i = nbr_idx[(int64_t)j * K + r];
                    if ((unsigned)i >= (unsigned)n_items) continue;
                    const int t = lower_bound_lds(tgi, NT, i);
                    if (t < NT && tgi[t] == i) atomicAdd((unsigned long long *)&tsc[t], (unsigned long long)(uint32_t)nbr_w[(int64_t)j * K + r]);
                }
            }
        }
        if (tid < NT) {                                         // a target inside the profile is masked
            int live = 1;
            if (mask_profile) {
                int64_t lo = ub, hi = ue;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (col[mid] < tgi[tid]) lo = mid + 1; else hi = mid;
                }
                live = !(lo < ue && col[lo] == tgi[tid]);
            }
            tlive[tid] = live;
            if (live) atomicAdd(&hdr[LIVE_T], 1);
            else rank[(int64_t)slot * NT + tgc[tid]] = -1;
        }
        __syncthreads();
        if (tid < NT && tlive[tid]) {
            int r = 0;
            for (int f = 0; f < NT; ++f) r += (tlive[f] && beats(tsc[f], tgi[f], tsc[tid], tgi[tid])) ? 1 : 0;
            ss[r] = tsc[tid], si[r] = tgi[tid], sc[r] = tgc[tid];
        }
        __syncthreads();
        nlive = hdr[LIVE_T];
    }

    int64_t mlo = ub;                                           // the profile's first entry not below the tile
    for (int t0 = 0; t0 < n_items; t0 += T) {
        const int t1 = min(t0 + T, n_items), tl = t1 - t0;
        __syncthreads();                                        // the previous tile's scan is over
        for (int i = tid; i < tl; i += kBlk) acc[i] = 0;
        __syncthreads();
        if constexpr (kUser) {
            for (int r = wv; r < K; r += kWaves) {              // uniform over the wave: the ballot below sees every lane
                int64_t c = cur[r];
                const int64_t e = cend[r];
                const unsigned long long w = cw[r];
                while (c < e) {
                    const int64_t p = c + lane;
                    const int i = p < e ? col[p] : INT_MAX;
                    const bool below = p < e && i < t1;         // the row is sorted: these lanes are a prefix of the chunk
                    if (below && (unsigned)(i - t0) < (unsigned)tl) atomicAdd((unsigned long long *)&acc[i - t0], w);
                    const int n = __popcll(__ballot(below));
                    c += n;
                    if (n < 64) break;                          // the chunk reached t1 or the row's end
                }
                if (lane == 0) cur[r] = c;                      // this wave alone reads and writes slot r
            }
        } else {
            for (int64_t p = ub + wv; p < ue; p += kWaves) {
                const int j = col[p];
                if ((unsigned)j >= (unsigned)n_items) continue;
                for (int r = lane; r < K; r += 64) {
                    const int i = nbr_idx[(int64_t)j * K + r];
                    if ((unsigned)(i - t0) < (unsigned)tl)
                        atomicAdd((unsigned long long *)&acc[i - t0], (unsigned long long)(uint32_t)nbr_w[(int64_t)j * K + r]);
                }
            }
        }
        __syncthreads();
        if (mask_profile) {                                     // the profile is sorted: its items inside the tile are [mlo, mhi)
            int64_t lo = mlo, hi = ue;
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (col[mid] < t1) lo = mid + 1; else hi = mid;
            }
            for (int64_t p = mlo + tid; p < lo; p += kBlk) {
                const int c = col[p];
                if ((unsigned)(c - t0) < (unsigned)tl) acc[c - t0] = -1;
            }
            mlo = lo;
            __syncthreads();
        }

        // the accumulators hold s(u, i) for the tile's items, -1 where excluded.  Count for the targets and count what would be appended.
        int64_t ts = 0;
        int ti = INT_MAX;
        bool has_thr = hdr[LIST_N] == N;
        if (has_thr) ts = es[N - 1], ti = ei[N - 1];
        int n = 0;
        for (int base = 0; base < tl; base += kBlk) {           // uniform trip count: the wave votes below see every lane
            const int i = base + tid, v = t0 + i;
            const int64_t s = i < tl ? acc[i] : -1;
            const bool cand = s >= 0;
            n += (cand && (!has_thr || beats(s, v, ts, ti))) ? 1 : 0;
            if (nlive > 0) {
                bool act = cand && beats(s, v, ss[nlive - 1], si[nlive - 1]);
                int p = nlive - 1;
                if (act) {                                      // the first sorted target this candidate beats
                    int lo = 0, hi = nlive - 1;
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (beats(s, v, ss[mid], si[mid])) hi = mid; else lo = mid + 1;
                    }
                    p = lo;
                }
                unsigned long long rem = __ballot(act);
                while (rem) {                                   // one add per distinct position in the wave
                    const int leader = __ffsll((long long)rem) - 1;
                    const int p0 = __shfl(p, leader);
                    const unsigned long long m = __ballot(act && p == p0);
                    if (lane == leader) atomicAdd(&hist[p0], __popcll(m));
                    rem &= ~m;
                }
            }
        }
        if (n) atomicAdd(&hdr[CAND], n);
        __syncthreads();
        const int cand = hdr[CAND], pn = hdr[PEND_N];
        __syncthreads();
        if (tid == 0) hdr[CAND] = 0;
        if (cand == 0) continue;
        // One piece when the tile's candidates fit the buffer; else pieces, merged after each.  While the list is not full there is no N-th entry
        // to refuse a candidate, so pieces are short (kBlk items) and pending entries are merged at once: a merge costs the square of what it
        // ranks, and the first one gives every later item a bound to fail against.
        bool whole = cand <= (has_thr ? kPend : kBlk);
        if (pn > 0 && (!whole || !has_thr || pn + cand > kPend)) {
            merge(hdr, es, ei, N);
            has_thr = hdr[LIST_N] == N;
            if (has_thr) ts = es[N - 1], ti = ei[N - 1];
            whole = cand <= (has_thr ? kPend : kBlk);
        }
        for (int base = 0; base < tl;) {                        // pieces start with an empty buffer; a whole tile with pn + cand <= kPend
            const int end = whole ? tl : min(base + (has_thr ? kPend : kBlk), tl);
            for (int i = base + tid; i < end; i += kBlk) {
                const int64_t s = acc[i];
                const int v = t0 + i;
                if (s < 0) continue;
                if (has_thr && !beats(s, v, ts, ti)) continue;
                const int w = atomicAdd(&hdr[PEND_N], 1);
                if (w < kPend) es[kMaxN + w] = s, ei[kMaxN + w] = v;
            }
            if (!whole) {
                __syncthreads();
                merge(hdr, es, ei, N);
                has_thr = hdr[LIST_N] == N;
                if (has_thr) ts = es[N - 1], ti = ei[N - 1];
            }
            base = end;
        }
    }
    __syncthreads();
    if (hdr[PEND_N] > 0) merge(hdr, es, ei, N);                 // uniform: nobody writes the word before the merge's first barrier
    const int ln = hdr[LIST_N];
    for (int j = tid; j < N; j += kBlk) oi[j] = j < ln ? ei[j] : -1, os[j] = j < ln ? es[j] : 0;
    if (tid < nlive) {                                          // candidates that beat the target at sorted position tid
        int c = 0;
        for (int p = 0; p <= tid; ++p) c += hist[p];
        rank[(int64_t)slot * NT + sc[tid]] = c;
    }
}

// the checks and the launch of both C entries; the lists have one row per item (item side) or per user (user side)
template <bool kUser>
int score_topk(const int64_t *rowptr, const int32_t *col, int64_t n_users, int64_t n_items, const int32_t *nbr_idx, const int32_t *nbr_w, int64_t k,
               const int32_t *rows, int64_t n_queries, int64_t n, int32_t mask_profile, const int32_t *tgt_id, const int32_t *tgt_col,
               int64_t n_targets, const int32_t *order, int64_t tile_items, int32_t *idx, int64_t *score, int32_t *rank, arl_stream_t stream) {
    constexpr int kFixed = kUser ? kUserFixedBytes : kFixedBytes, kTileMax = kUser ? kUserMaxTile : kMaxTile;
    constexpr int kTileDefault = kUser ? kUserDefaultTile : kDefaultTile;
    if (n_users < 0 || n_items < 0 || n_queries < 0 || k < 1 || n < 1 || n_targets < 0 || tile_items < 0) return ARL_E_ARG;
    if (k > kMaxK || n > kMaxN || n_targets > kMaxT || tile_items > kTileMax) return ARL_E_RANGE;
    if (n_users > 0x7fffffffll || n_items > 0x7fffffffll || n_queries > 0x7fffffffll) return ARL_E_RANGE;
    if (n_queries * n > 0x7fffffffll || n_queries * n_targets > 0x7fffffffll) return ARL_E_RANGE;
    if (n_queries == 0) return ARL_OK;
    if (!rowptr || !idx || !score) return ARL_E_NULL;           // col may be NULL for a matrix without entries
    if ((kUser ? n_users : n_items) > 0 && (!nbr_idx || !nbr_w)) return ARL_E_NULL;
    if (n_targets > 0 && (!tgt_id || !tgt_col || !rank)) return ARL_E_NULL;
    int64_t T = tile_items ? tile_items : kTileDefault;
    if (T > n_items) T = n_items > 0 ? n_items : 1;
    const size_t shm = (size_t)kFixed + 8 * (size_t)((T + 1) & ~1ll);
    const void *fn = (const void *)knn_score_topk_kernel<kUser>;
    if (shm > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return (int)e;
    }
    const dim3 grid((unsigned)n_queries), block(kBlk);
    hipLaunchKernelGGL(knn_score_topk_kernel<kUser>, grid, block, shm, (hipStream_t)stream, rowptr, col, nbr_idx, nbr_w, rows, order, tgt_id, tgt_col,
                       (int)n_users, (int)n_items, (int)n_queries, (int)k, (int)n, (int)n_targets, mask_profile ? 1 : 0, (int)T, idx, score, rank);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_itemknn_max_k(void) { return kMaxK; }
int64_t arl_itemknn_max_n(void) { return kMaxN; }
int64_t arl_itemknn_max_targets(void) { return kMaxT; }
int64_t arl_itemknn_max_tile_items(void) { return kMaxTile; }
int64_t arl_itemknn_default_tile_items(void) { return kDefaultTile; }

int arl_itemknn_score_topk_i64(const int64_t *rowptr, const int32_t *col, int64_t n_users, int64_t n_items, const int32_t *nbr_idx,
                               const int32_t *nbr_w, int64_t k, const int32_t *rows, int64_t n_queries, int64_t n, int32_t mask_profile,
                               const int32_t *tgt_id, const int32_t *tgt_col, int64_t n_targets, const int32_t *order, int64_t tile_items,
                               int32_t *idx, int64_t *score, int32_t *rank, arl_stream_t stream) {
    return score_topk<false>(rowptr, col, n_users, n_items, nbr_idx, nbr_w, k, rows, n_queries, n, mask_profile, tgt_id, tgt_col, n_targets, order,
                             tile_items, idx, score, rank, stream);
}

int64_t arl_userknn_max_tile_items(void) { return kUserMaxTile; }
int64_t arl_userknn_default_tile_items(void) { return kUserDefaultTile; }

int arl_userknn_score_topk_i64(const int64_t *rowptr, const int32_t *col, int64_t n_users, int64_t n_items, const int32_t *nbr_idx,
                               const int32_t *nbr_w, int64_t k, const int32_t *rows, int64_t n_queries, int64_t n, int32_t mask_profile,
                               const int32_t *tgt_id, const int32_t *tgt_col, int64_t n_targets, const int32_t *order, int64_t tile_items,
                               int32_t *idx, int64_t *score, int32_t *rank, arl_stream_t stream) {
    return score_topk<true>(rowptr, col, n_users, n_items, nbr_idx, nbr_w, k, rows, n_queries, n, mask_profile, tgt_id, tgt_col, n_targets, order,
                            tile_items, idx, score, rank, stream);
}

}  // extern "C"

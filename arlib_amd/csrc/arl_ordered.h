// arl_ordered.h -- the ownership scan of the ordered (atomic-free) accumulations, shared by arl_kernels.hip and arl_advpair.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

// ---- ordered accumulation (no float atomics): dst[idx[t]] += scale * src[t], duplicates summed in ascending t.
// One wave per contribution t of the window [c0, c1).  The wave scans the window's index list 256 entries per trip (coalesced; the list is a
// few KB and stays in L1): if an EARLIER entry names the same row the wave exits -- the first entry of a row is its owner -- otherwise it
// adds the row's contributions one after the other in index order, starting from the value already in dst.  That is the association of CPU
// index_put_(accumulate=True), i.e. of the reference's gathers under autograd (recommender/LightGCN.py:51-56, util/loss.py:5-9), and it
// is bit-identical from run to run.  Work is O(n^2 / 64) wave-trips, so a launch covers at most kOrderedWindow entries; longer lists run
// as successive launches (stream order keeps the result deterministic).
constexpr int kOrderedWindow = 16384;

// Scan of the window by one wave: `on_hit(tt)` runs, in ascending tt, for every entry tt whose row (`rowof(tt)`) equals `row`.  Returns false --
// the wave must exit -- as soon as an entry BEFORE t names the row (that entry's wave owns it).
template <class RowOf, class OnHit>
__device__ __forceinline__ bool ordered_scan(int c0, int c1, int t, long long row, int lane, RowOf rowof, OnHit on_hit) {
    for (int base = c0; base < c1; base += 256) {
        long long v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = base + 64 * i + lane;
            v[i] = j < c1 ? (long long)rowof(j) : -1ll;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned long long m = __ballot(v[i] == row);
            const int b0 = base + 64 * i;
            if (b0 < t) {
                const int lim = t - b0;
                if (lim >= 64 ? m != 0ull : (m & ((1ull << lim) - 1ull)) != 0ull) return false;
            }
            while (m) {
                const int tt = b0 + __ffsll((long long)m) - 1;
                m &= m - 1ull;
                on_hit(tt);
            }
        }
    }
    return true;
}

// The same scan over a copy of the window's rows in LDS (staged once per workgroup by stage_rows): one dependent global-memory latency per
// 256 entries becomes an LDS read -- the scan of a 6 144-entry batch list drops from ~10 us to ~1 us per wave.
template <class OnHit>
__device__ __forceinline__ bool ordered_scan_lds(const int32_t *srows, int c0, int c1, int t, int row, int lane, OnHit on_hit) {
    const int n = c1 - c0, tl = t - c0;
    for (int base = 0; base < n; base += 512) {
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = base + 64 * i + lane;
            v[i] = j < n ? srows[j] : -1;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            unsigned long long m = __ballot(v[i] == row);
            const int b0 = base + 64 * i;
            if (b0 < tl) {
                const int lim = tl - b0;
                if (lim >= 64 ? m != 0ull : (m & ((1ull << lim) - 1ull)) != 0ull) return false;
            }
            while (m) {
                const int tt = c0 + b0 + __ffsll((long long)m) - 1;
                m &= m - 1ull;
                on_hit(tt);
            }
        }
    }
    return true;
}
// group form: `on_group(m, g0)` receives the 64-bit hit mask of entries g0 .. g0 + 63 (absolute indices), groups in ascending order
template <class OnGroup>
__device__ __forceinline__ bool ordered_scan_lds_groups(const int32_t *srows, int c0, int c1, int t, int row, int lane, OnGroup on_group) {
    const int n = c1 - c0, tl = t - c0;
    for (int base = 0; base < n; base += 512) {
        int v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = base + 64 * i + lane;
            v[i] = j < n ? srows[j] : -1;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const unsigned long long m = __ballot(v[i] == row);
            const int b0 = base + 64 * i;
            if (b0 < tl) {
                const int lim = tl - b0;
                if (lim >= 64 ? m != 0ull : (m & ((1ull << lim) - 1ull)) != 0ull) return false;
            }
            if (m) on_group(m, c0 + b0);
        }
    }
    return true;
}

}  // namespace

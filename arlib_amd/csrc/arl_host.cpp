// arl_host.cpp -- host side of libarlib_amd.so: the bit-exact BPR pair sampler.
//
// Replaces util/sampler.py:4-30 (next_batch_pairwise).  The reference draws from CPython's global
// `random` (MT19937, seeded by util/tool.py:101-108).  To stay a drop-in, the caller hands us
// random.getstate()[1] (624 words + index), we advance it exactly as CPython would, and the caller
// puts it back with random.setstate().  Sequential by nature (rejection loops consume a
// data-dependent number of draws), so this lives on the host and feeds the GPU through pinned
// buffers; it costs ~10 ns per draw versus ~2.5 us per sample in the reference's Python loop.
#include <cstdint>
#include <cstddef>
#include <queue>
#include <cmath>
#include <algorithm>
#include <utility>
#include <vector>
#include "arlib_amd.h"

namespace {

// View over a CPython MT19937 state vector (624 words followed by the read position).
class PyMersenne {
public:
    explicit PyMersenne(uint32_t *state) : w_(state), pos_(state[kN]) {}
    ~PyMersenne() { w_[kN] = pos_; }

    uint32_t next32() {
        if (pos_ >= kN) refill();
        uint32_t y = w_[pos_++];
        y ^= y >> 11;
        y ^= (y << 7) & 0x9d2c5680u;
        y ^= (y << 15) & 0xefc60000u;
        return y ^ (y >> 18);
    }

    // Random._randbelow_with_getrandbits for n < 2^32: draw bit_length(n) top bits until < n.
    uint32_t below(uint32_t n) {
        if (n == 0) return 0;
        const int shift = __builtin_clz(n);          // 32 - bit_length(n)
        uint32_t r;
        do { r = next32() >> shift; } while (r >= n);
        return r;
    }

    static void seed_by_array(uint32_t *w, const uint32_t *key, int64_t len) {
        w[0] = 19650218u;
        for (uint32_t i = 1; i < kN; ++i) w[i] = 1812433253u * (w[i - 1] ^ (w[i - 1] >> 30)) + i;
        uint32_t i = 1;
        int64_t j = 0;
        for (int64_t k = (len > (int64_t)kN ? len : (int64_t)kN); k > 0; --k) {
            w[i] = (w[i] ^ ((w[i - 1] ^ (w[i - 1] >> 30)) * 1664525u)) + key[j] + (uint32_t)j;
            if (++i >= kN) { w[0] = w[kN - 1]; i = 1; }
            if (++j >= len) j = 0;
        }
        for (uint32_t k = kN - 1; k > 0; --k) {
            w[i] = (w[i] ^ ((w[i - 1] ^ (w[i - 1] >> 30)) * 1566083941u)) - i;
            if (++i >= kN) { w[0] = w[kN - 1]; i = 1; }
        }
        w[0] = 0x80000000u;
        w[kN] = kN;
    }

private:
    static constexpr uint32_t kN = 624, kM = 397;
    static uint32_t twist(uint32_t hi, uint32_t lo, uint32_t far) {
        const uint32_t y = (hi & 0x80000000u) | (lo & 0x7fffffffu);
        return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    void refill() {
        for (uint32_t k = 0; k < kN - kM; ++k) w_[k] = twist(w_[k], w_[k + 1], w_[k + kM]);
        for (uint32_t k = kN - kM; k < kN - 1; ++k) w_[k] = twist(w_[k], w_[k + 1], w_[k + kM - kN]);
        w_[kN - 1] = twist(w_[kN - 1], w_[0], w_[kM - 1]);
        pos_ = 0;
    }
    uint32_t *w_;
    uint32_t pos_;
};

// `item in training_set_u[user]` on the CSR image of the dict-of-dicts (sorted item ids per user).
inline bool user_has_item(const int64_t *rowptr, const int32_t *items, int64_t rows, int32_t user, int32_t item) {
    if (user < 0 || user >= rows) return false;
    const int32_t *lo = items + rowptr[user], *hi = items + rowptr[user + 1];
    while (lo < hi) {
        const int32_t *mid = lo + (hi - lo) / 2;
        if (*mid < item) lo = mid + 1; else hi = mid;
    }
    return lo < items + rowptr[user + 1] && *lo == item;
}

}  // namespace

extern "C" {

int arl_abi_version(void) { return 34; }

int arl_mt_seed(uint32_t *mt_state, const uint32_t *key, int64_t key_len) {
    if (!mt_state || !key) return ARL_E_NULL;
    if (key_len < 1) return ARL_E_ARG;
    PyMersenne::seed_by_array(mt_state, key, key_len);
    return ARL_OK;
}

int arl_sampler_shuffle(uint32_t *mt_state, int32_t *pairs, int64_t nnz) {
    if (!mt_state || (!pairs && nnz > 0)) return ARL_E_NULL;
    if (nnz < 0 || nnz > 0xFFFFFFFFll) return ARL_E_RANGE;
    if (mt_state[624] > 624) return ARL_E_ARG;
    PyMersenne rng(mt_state);
    // random.shuffle: for i in reversed(range(1, n)): j = randbelow(i + 1); x[i], x[j] = x[j], x[i]
    int64_t *rows = reinterpret_cast<int64_t *>(pairs);      // one (user,item) pair = 8 bytes
    const bool aligned = (reinterpret_cast<uintptr_t>(pairs) & 7u) == 0;
    // The partner indices depend on the generator alone, not on the swaps: they are drawn a block ahead and their rows prefetched, then the swaps run in
    // the reference's order.  (32 M pairs = 256 MB: every swap partner is a cache miss; 0.45 -> ~0.2 s per cfg2 epoch, the serial part of device_epoch.)
    constexpr int kAhead = 512;
    int64_t js[kAhead];
    for (int64_t i = nnz - 1; i >= 1;) {
        const int cnt = (int)(i < kAhead ? i : kAhead);               // swaps i, i - 1, ..., i - cnt + 1 (all >= 1)
        for (int t = 0; t < cnt; ++t) {
            js[t] = rng.below((uint32_t)(i - t + 1));
            __builtin_prefetch(pairs + 2 * js[t], 1, 0);
        }
        if (aligned) {
            for (int t = 0; t < cnt; ++t) { const int64_t a = i - t, j = js[t], v = rows[a]; rows[a] = rows[j]; rows[j] = v; }
        } else {
            for (int t = 0; t < cnt; ++t)
                for (int c = 0; c < 2; ++c) { const int64_t a = i - t, j = js[t]; const int32_t v = pairs[2 * a + c]; pairs[2 * a + c] = pairs[2 * j + c]; pairs[2 * j + c] = v; }
        }
        i -= cnt;
    }
    return ARL_OK;
}

int arl_mt_sample_range(uint32_t *mt_state, int64_t n, int64_t k, int32_t use_pool, int32_t *out, int32_t *scratch) {
    // random.sample(range(n), k) of CPython 3.10 (Lib/random.py:sample): the pool form when the caller's set-size rule says so
    // (scratch: n int32), rejection against the already selected values otherwise (scratch: (n + 31) / 32 words, zeroed here).
    if (!mt_state || (!out && k > 0) || !scratch) return ARL_E_NULL;
    if (n < 0 || k < 0 || k > n || n > 0x7FFFFFFFll) return ARL_E_ARG;
    if (mt_state[624] > 624) return ARL_E_ARG;
    PyMersenne rng(mt_state);
    if (use_pool) {
        for (int64_t i = 0; i < n; ++i) scratch[i] = (int32_t)i;
        for (int64_t i = 0; i < k; ++i) {
            const uint32_t j = rng.below((uint32_t)(n - i));
            out[i] = scratch[j];
            scratch[j] = scratch[n - i - 1];
        }
    } else {
        uint32_t *seen = reinterpret_cast<uint32_t *>(scratch);
        for (int64_t w = 0; w < (n + 31) / 32; ++w) seen[w] = 0u;
        for (int64_t i = 0; i < k; ++i) {
            uint32_t j = rng.below((uint32_t)n);
            while ((seen[j >> 5] >> (j & 31)) & 1u) j = rng.below((uint32_t)n);
            seen[j >> 5] |= 1u << (j & 31);
            out[i] = (int32_t)j;
        }
    }
    return ARL_OK;
}

}  // extern "C"

// ---- GOAT's itemSample (reference attack/Gray/GOAT.py:105-135) ----
namespace {

// The r-th (0-based) id of range(n) minus the ascending, duplicate-free ids excl[0..n_excl): r plus the number of excluded ids at or below it.
// excl[t] - t never decreases, so the count is the first t with excl[t] - t > r.
inline int32_t nth_remaining(int64_t r, const int32_t *excl, int64_t n_excl) {
    int64_t lo = 0, hi = n_excl;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)excl[mid] - mid <= r) lo = mid + 1; else hi = mid;
    }
    return (int32_t)(r + lo);
}

// random.sample(pool, m) of CPython 3.10 for the pool above (n ids), written to out[0..m).  idx: n int32 (pool form), seen: (n + 31) / 32 words,
// all zero on entry and on return (selection form).
void sample_remaining(PyMersenne &rng, int64_t n, int64_t m, const int32_t *excl, int64_t n_excl, int32_t *out, int32_t *idx, uint32_t *seen) {
    int64_t setsize = 21;
    if (m > 5) {
        const double e = std::ceil(std::log((double)(m * 3)) / std::log(4.0));       // math.log(k * 3, 4) = log(x) / log(4)
        int64_t p = 1;
        for (int64_t t = 0; t < (int64_t)e; ++t) p *= 4;
        setsize += p;
    }
    if (n <= setsize) {
        for (int64_t i = 0; i < n; ++i) idx[i] = (int32_t)i;
        for (int64_t i = 0; i < m; ++i) {
            const uint32_t j = rng.below((uint32_t)(n - i));
            out[i] = nth_remaining(idx[j], excl, n_excl);
            idx[j] = idx[n - i - 1];
        }
    } else {
        for (int64_t i = 0; i < m; ++i) {
            uint32_t j = rng.below((uint32_t)n);
            while ((seen[j >> 5] >> (j & 31)) & 1u) j = rng.below((uint32_t)n);
            seen[j >> 5] |= 1u << (j & 31);
            idx[i] = (int32_t)j;                                                      // remembered to clear its bit below
            out[i] = nth_remaining(j, excl, n_excl);
        }
        for (int64_t i = 0; i < m; ++i) seen[(uint32_t)idx[i] >> 5] = 0u;
    }
}

// sorted, duplicate-free union of a (sorted, duplicate-free, na ids) and b (nb ids in any order, sorted in place) into dst; returns its length
int64_t merge_sorted(const int32_t *a, int64_t na, int32_t *b, int64_t nb, int32_t *dst) {
    std::sort(b, b + nb);
    int64_t i = 0, j = 0, n = 0;
    while (i < na || j < nb) {
        int32_t v;
        if (j >= nb || (i < na && a[i] <= b[j])) v = a[i++]; else v = b[j++];
        if (n == 0 || dst[n - 1] != v) dst[n++] = v;
    }
    return n;
}

}  // namespace

extern "C" {

int64_t arl_goat_item_sample_scratch_words(int64_t n_items, int64_t k, int64_t n_targets) {
    if (n_items < 0 || k < 0 || n_targets < 0) return ARL_E_ARG;
    return n_items + (n_items + 31) / 32 + 4 * (k + n_targets) + 16;
}

int arl_goat_item_sample(uint32_t *mt_state, const int64_t *rowptr, const int32_t *items, int64_t n_users, int64_t n_items,
                         const double *int_num, const int32_t *targets, int64_t n_targets, int64_t n_fake, int64_t k, double min_items,
                         int64_t thr, int32_t *out_s, int32_t *out_f, uint8_t *out_real, int32_t *out_user, int32_t *scratch) {
    if (!mt_state || !rowptr || !int_num || !out_user || !scratch || (n_targets > 0 && !targets)) return ARL_E_NULL;
    if (n_users < 1 || n_items < 1 || n_targets < 0 || n_fake < 0 || k < 1) return ARL_E_ARG;
    if (n_users > 0x7fffffffll || n_items > 0x7fffffffll) return ARL_E_RANGE;
    if ((double)(k + n_targets) > 0.4 * (double)n_items) return ARL_E_RANGE;          // past it CPython's set no longer iterates in ascending order
    if (mt_state[624] > 624) return ARL_E_ARG;
    const int64_t ks = (int64_t)((double)k * 0.3), kf_walk = (int64_t)((double)k * 0.7), kf = k - ks;       // int(k * 0.3), int(k * 0.7)
    if (n_fake > 0 && ((ks > 0 && !out_s) || !out_f || !out_real)) return ARL_E_NULL;
    for (int64_t t = 0; t < n_targets; ++t)
        if (targets[t] < 0 || targets[t] >= n_items) return ARL_E_ARG;
    // scratch: idx [n_items] | seen [(n_items + 31) / 32] | base, excl, walk, tmp [k + n_targets each]
    const int64_t cap = k + n_targets;
    int32_t *idx = scratch;
    uint32_t *seen = reinterpret_cast<uint32_t *>(scratch + n_items);
    int32_t *base = scratch + n_items + (n_items + 31) / 32, *excl = base + cap, *walk = excl + cap, *tmp = walk + cap;
    for (int64_t w = 0; w < (n_items + 31) / 32; ++w) seen[w] = 0u;
    PyMersenne rng(mt_state);
    out_user[0] = -1;
    if (n_fake == 0) return ARL_OK;

    // while realUser.sum() < O_u * itemNum: realUser = interact[randint(0, U - 1)] -- realUser is reset per call, so only the first row draws.
    // The reference never returns when no user has that many items; here that is an argument error, found before anything is drawn.
    if (min_items > 0.0) {
        bool any = false;
        for (int64_t u = 0; u < n_users && !any; ++u) any = (double)(rowptr[u + 1] - rowptr[u]) >= min_items;
        if (!any) return ARL_E_ARG;
    }
    int32_t user = -1;
    double have = 0.0;
    while (have < min_items) {
        user = (int32_t)rng.below((uint32_t)n_users);
        have = (double)(rowptr[user + 1] - rowptr[user]);
    }
    out_user[0] = user;
    const int32_t *ub = user >= 0 ? items + rowptr[user] : nullptr, *ue = user >= 0 ? items + rowptr[user + 1] : nullptr;
    // the walk over the real user's items: I_s first, else (`elif`) I_f; walk[0..ns) = I_s, walk[ns..ns + nf) = I_f
    int64_t ns = 0, nf = 0;
    const double thr_s = (double)thr, thr_f = (double)thr / 3.0;
    for (const int32_t *p = ub; p < ue; ++p) {
        if (*p < 0 || *p >= n_items) continue;
        if (int_num[*p] > thr_s && ns < ks) walk[ns++] = *p;
        else if (int_num[*p] > thr_f && nf < kf_walk) tmp[nf++] = *p;
    }
    for (int64_t t = 0; t < nf; ++t) walk[ns + t] = tmp[t];
    if (ns + nf > k) return ARL_E_ARG;                                                // cannot happen: int(0.3 k) + int(0.7 k) <= k
    // base = sorted union of the targets and the walk's items
    for (int64_t t = 0; t < n_targets; ++t) tmp[t] = targets[t];
    const int64_t nt = merge_sorted(nullptr, 0, tmp, n_targets, excl);
    for (int64_t t = 0; t < ns + nf; ++t) tmp[t] = walk[t];
    const int64_t n_base = merge_sorted(excl, nt, tmp, ns + nf, base);

    for (int64_t f = 0; f < n_fake; ++f) {
        int32_t *rs = out_s + f * ks, *rf = out_f + f * kf;
        for (int64_t t = 0; t < ns; ++t) rs[t] = walk[t];
        for (int64_t t = 0; t < nf; ++t) rf[t] = walk[ns + t];
        const int32_t *ex = base;
        int64_t n_ex = n_base;
        if (ns < ks) {                                                                 // while len(I_s) < int(k * 0.3): one random.sample fills it
            sample_remaining(rng, n_items - n_ex, ks - ns, ex, n_ex, rs + ns, idx, seen);
            for (int64_t t = ns; t < ks; ++t) tmp[t - ns] = rs[t];
            n_ex = merge_sorted(base, n_base, tmp, ks - ns, excl);
            ex = excl;
        }
        if (nf < kf)                                                                   // while len(I_f) + len(I_s) < k
            sample_remaining(rng, n_items - n_ex, kf - nf, ex, n_ex, rf + nf, idx, seen);
        uint8_t *rr = out_real + f * k;                                                // realUser[I_s + I_f]
        for (int64_t t = 0; t < k; ++t) {
            const int32_t it = t < ks ? rs[t] : rf[t - ks];
            rr[t] = (ub && std::binary_search(ub, ue, it)) ? 1 : 0;
        }
    }
    return ARL_OK;
}

int arl_sampler_next_batch(uint32_t *mt_state, const int32_t *pairs, int64_t begin, int64_t count, int32_t n_items,
                           const int64_t *memb_rowptr, const int32_t *memb_items, int64_t memb_rows,
                           int32_t *out_u, int32_t *out_p, int32_t *out_n) {
    if (!mt_state || !pairs || !out_u || !out_p || !out_n) return ARL_E_NULL;
    if (memb_rows > 0 && (!memb_rowptr || !memb_items)) return ARL_E_NULL;
    if (begin < 0 || count < 0 || n_items <= 0) return ARL_E_ARG;
    if (mt_state[624] > 624) return ARL_E_ARG;
    PyMersenne rng(mt_state);
    for (int64_t b = 0; b < count; ++b) {
        const int32_t user = pairs[2 * (begin + b)], pos = pairs[2 * (begin + b) + 1];
        int32_t neg;
        do { neg = (int32_t)rng.below((uint32_t)n_items); }
        while (user_has_item(memb_rowptr, memb_items, memb_rows, user, neg));
        out_u[b] = user; out_p[b] = pos; out_n[b] = neg;
    }
    return ARL_OK;
}

// Plan helper of the register-blocked SpMM: longest-processing-time dealing.  Rows arrive sorted by weight (edge count),
// heaviest first; each goes to the least loaded bin (wave) that still has a free slot; ties go to the lowest bin id, so the
// plan is reproducible.  n_bins * cap >= n is required.
int arl_lpt_deal(int64_t n, const int32_t *weight_desc, int64_t n_bins, int64_t cap, int32_t *bin_out, int32_t *slot_out) {
    if (n < 0 || n_bins < 0 || cap < 1 || n_bins > 0x7fffffffll || n_bins * cap < n) return ARL_E_ARG;
    if (n == 0) return ARL_OK;
    if (!weight_desc || !bin_out || !slot_out) return ARL_E_NULL;
    typedef std::pair<int64_t, int32_t> Load;                      // (edges so far, bin)
    std::priority_queue<Load, std::vector<Load>, std::greater<Load>> open;
    std::vector<int32_t> fill((size_t)n_bins, 0);
    for (int64_t b = 0; b < n_bins; ++b) open.push(Load(0, (int32_t)b));
    for (int64_t r = 0; r < n; ++r) {
        if (weight_desc[r] < 0 || (r > 0 && weight_desc[r] > weight_desc[r - 1])) return ARL_E_ARG;
        const Load top = open.top();
        open.pop();
        bin_out[r] = top.second;
        slot_out[r] = fill[top.second]++;
        if (fill[top.second] < cap) open.push(Load(top.first + weight_desc[r], top.second));
    }
    return ARL_OK;
}

// ---- SYN-v1: the synthetic interaction graphs of the benchmark, generated natively.  Every random number is a counter-based hash
//   h(stream, index) = splitmix64(splitmix64(seed ^ stream * PHI) ^ index)
// so this generator and the numpy one (arlib_amd/util/synthetic.py) emit the same pair list, checked by arl_graph_digest.
static inline uint64_t syn_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
static inline uint64_t syn_hash(uint64_t base, uint64_t index) { return syn_splitmix64(index ^ base); }
static inline uint64_t syn_base(uint64_t seed, uint64_t stream) { return syn_splitmix64(seed ^ (stream * 0x9E3779B97F4A7C15ull)); }
static inline double syn_uniform(uint64_t h) { return ((double)(h >> 11) + 0.5) * (1.0 / 9007199254740992.0); }

/* Writes the user-major sorted, de-duplicated (user, item) pairs into pairs_out [capacity][2] and returns their number (or the number
 * needed, without writing, when pairs_out is NULL or capacity is too small); negative = argument error. */
int64_t arl_syn_v1_pairs(int64_t n_users, int64_t n_items, double mean_deg, uint64_t seed, double sigma, int64_t deg_min, int64_t deg_max,
                         int32_t *pairs_out, int64_t capacity) {
    if (n_users <= 0 || n_items <= 0 || n_users > 0x7fffffffll || n_items > 0x7fffffffll || !(mean_deg > 0) || !(sigma >= 0) || deg_min < 0 || deg_max < deg_min)
        return ARL_E_ARG;
    const uint64_t b1 = syn_base(seed, 1), b2 = syn_base(seed, 2), b3 = syn_base(seed, 3), b4 = syn_base(seed, 4), b5 = syn_base(seed, 5);
    const double mu = std::log(mean_deg) - 0.5 * sigma * sigma;
    const double two_pi = 2.0 * 3.14159265358979323846;
    const int64_t hi = deg_max < n_items ? deg_max : n_items;
    std::vector<int64_t> deg((size_t)n_users);
    int64_t total = 0;
    for (int64_t u = 0; u < n_users; ++u) {
        const double u1 = syn_uniform(syn_hash(b1, (uint64_t)u)), u2 = syn_uniform(syn_hash(b2, (uint64_t)u));
        const double z = std::sqrt(-2.0 * std::log(u1)) * std::cos(two_pi * u2);
        double dg = std::nearbyint(std::exp(mu + sigma * z));          // numpy rint: round half to even (default FP environment)
        if (dg < (double)deg_min) dg = (double)deg_min;
        if (dg > (double)hi) dg = (double)hi;
        deg[(size_t)u] = (int64_t)dg;
        total += deg[(size_t)u];
    }
    // pi = stable argsort of h(4, j)
    std::vector<std::pair<uint64_t, int64_t>> hp((size_t)n_items);
    for (int64_t j = 0; j < n_items; ++j) hp[(size_t)j] = std::make_pair(syn_hash(b4, (uint64_t)j), j);
    std::stable_sort(hp.begin(), hp.end(), [](const std::pair<uint64_t, int64_t> &a, const std::pair<uint64_t, int64_t> &b) { return a.first < b.first; });
    std::vector<int64_t> keys;
    keys.reserve((size_t)(total + n_items));
    int64_t k = 0;
    for (int64_t u = 0; u < n_users; ++u)
        for (int64_t t = 0; t < deg[(size_t)u]; ++t, ++k) {
            const double r = syn_uniform(syn_hash(b3, (uint64_t)k));
            int64_t pos = (int64_t)((double)n_items * r * r);
            if (pos > n_items - 1) pos = n_items - 1;
            keys.push_back(u * n_items + hp[(size_t)pos].second);
        }
    for (int64_t j = 0; j < n_items; ++j) keys.push_back((int64_t)(syn_hash(b5, (uint64_t)j) % (uint64_t)n_users) * n_items + j);      // no isolated item
    std::sort(keys.begin(), keys.end());
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    const int64_t nnz = (int64_t)keys.size();
    if (!pairs_out || capacity < nnz) return nnz;
    for (int64_t e = 0; e < nnz; ++e) {
        pairs_out[2 * e] = (int32_t)(keys[(size_t)e] / n_items);
        pairs_out[2 * e + 1] = (int32_t)(keys[(size_t)e] % n_items);
    }
    return nnz;
}

/* Order-sensitive 64-bit digest of a pair list (the numpy twin is synthetic.graph_digest). */
uint64_t arl_graph_digest(const int32_t *pairs, int64_t n) {
    uint64_t acc = 0;
    if (pairs)
        for (int64_t e = 0; e < n; ++e) {
            const uint64_t a = (uint64_t)(int64_t)pairs[2 * e], b = (uint64_t)(int64_t)pairs[2 * e + 1];
            acc ^= syn_splitmix64((a * 0x100000001B3ull) ^ syn_splitmix64(b) ^ (uint64_t)e);
        }
    return acc ^ (uint64_t)(n > 0 ? n : 0);
}

}  // extern "C"

// arl_als.hip -- alternating least squares for implicit-feedback matrix factorisation (WRMF as published: Hu, Koren, Volinsky, ICDM'08) on gfx950:
// the Gram matrix of a table, the exact row update given the other table, and the objective, without any U x I tensor and without a stack of d x d
// matrices in memory.
//
// With p_ui = 1 on the stored entries, confidence c_ui = 1 + alpha w_ui (w = 1 or the stored value) and every other pair weighted 1:
//     L   = sum_u sum_i c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2)                       over ALL (u, i)
//     G   = Y^T Y
//     A_r = G + alpha sum_{i in P_r} w_ri y_i y_i^T + lambda I,   b_r = sum_{i in P_r} (1 + alpha w_ri) y_i,   x_r = A_r^-1 b_r
//     L   = sum_u [ x_u^T G x_u + sum_{i in P_u} ((1 + alpha w)(1 - s)^2 - s^2) ] + lambda (|X|^2 + |Y|^2),   s = x_u . y_i
//
// Rules kept throughout, those of arl_multinomial.hip / arl_kmeans.hip:
//   * S_r = sum w y y^T runs exact fp32 on v_mfma_f32_16x16x4_f32, lower-triangular 16 x 16 tiles only, the tiles dealt over the four waves of the
//     row's workgroup (at d = 128 nine tiles per wave: nothing spills); the row's entries pass through LDS 64 at a time (double-buffered gather);
//     a stage's 64 entries are summed in fp32 in list order, the stages in double;
//   * A_r is completed with G and lambda in double, factorised (Cholesky, lower, packed in LDS) and solved in double; b_r travels through the
//     factorisation as one more row, so the forward substitution is free;
//   * rows longer than split_len are cut into pieces; a piece's (S, b) is written by one workgroup (fp32 tiles, double b) and the row's workgroup adds
//     the pieces in piece order, in double, before it solves;
//   * no atomics: every word has one writer, sums have a fixed order, so the outputs are bit-identical from run to run;
//   * every workspace and output word is written before it is read; an empty row yields exactly 0.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_util.h"

namespace {

constexpr int kBlk = 256, kWaves = 4, kStage = 64;
constexpr int kDefaultSplit = 8192;
constexpr int kDefaultColSplit = 1024;                   // the adjoint's column pass: columns longer than this are cut into pieces
constexpr int kGramSpans = 256, kGramSpanRows = 128, kGramStage = 32;
constexpr int kPlanBlk = 1024;
constexpr int kSumParts = 256;
typedef float f32x4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ Gram
// part [span][D * D] = sum over the span's rows, ascending, of y y^T in double (an fp32 product is exact in double).  Thread (ty, tx) owns the
// elements (ty + 16 a, tx + 16 b): G[i][j] and G[j][i] add the same products in the same order, so G is symmetric bit for bit.
template <int D>
__global__ __launch_bounds__(kBlk) void als_gram_partial_kernel(const float *__restrict__ Y, int n, int span, double *__restrict__ part) {
    constexpr int R = D / 16, Q = D / 4;
    __shared__ float tile[kGramStage * D];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int r_begin = blockIdx.x * span, r_end = min(n, r_begin + span);
    double acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) acc[a][b] = 0.0;
    for (int r0 = r_begin; r0 < r_end; r0 += kGramStage) {
        for (int idx = tid; idx < kGramStage * Q; idx += kBlk) {
            const int row = idx / Q, q = (idx % Q) * 4;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);                     // rows past the span add exact zeros
            if (r0 + row < r_end) v = *reinterpret_cast<const float4 *>(Y + (size_t)(r0 + row) * D + q);
            *reinterpret_cast<float4 *>(&tile[row * D + q]) = v;
        }
        __syncthreads();
        for (int rr = 0; rr < kGramStage; ++rr) {
            double ya[R], yb[R];
#pragma unroll
            for (int a = 0; a < R; ++a) { ya[a] = (double)tile[rr * D + ty + 16 * a]; yb[a] = (double)tile[rr * D + tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) acc[a][b] += ya[a] * yb[b];
        }
        __syncthreads();
    }
    double *out = part + (size_t)blockIdx.x * D * D;
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) out[(ty + 16 * a) * D + tx + 16 * b] = acc[a][b];
}

__global__ __launch_bounds__(kBlk) void als_gram_fold_kernel(const double *__restrict__ part, int ns, int dd, double *__restrict__ G) {
    const int e = blockIdx.x * kBlk + threadIdx.x;
    if (e >= dd) return;
    double v = part[e];
    for (int s = 1; s < ns; ++s) v += part[(size_t)s * dd + e];
    G[e] = v;
}

struct gram_split { int ns, span; };
gram_split gram_splits(int64_t n) {
    int64_t s = (n + kGramSpanRows - 1) / kGramSpanRows;
    if (s > kGramSpans) s = kGramSpans;
    if (s < 1) s = 1;
    const int64_t span = (n + s - 1) / s;
    return gram_split{(int)((n + span - 1) / span), (int)span};
}

// ------------------------------------------------------------------------------------------------ the piece plan
// piece_off [n_solve + 1]: the exclusive prefix sum of the listed rows' piece counts, ceil(len / split_len) for a row longer than split_len and 0
// for every other row.  One workgroup: each thread sums a contiguous run of rows, the run sums are scanned in LDS.
__device__ __forceinline__ int als_row_len(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ rows, int j) {
    const int r = rows ? rows[j] : j;
    return rowptr[r + 1] - rowptr[r];
}

__global__ __launch_bounds__(kPlanBlk) void als_plan_kernel(const int32_t *__restrict__ rowptr, const int32_t *__restrict__ rows, int n_solve, int split_len,
                                                            int32_t *__restrict__ piece_off) {
    __shared__ int sums[kPlanBlk];
    const int tid = threadIdx.x;
    const int run = (n_solve + kPlanBlk - 1) / kPlanBlk;
    const int j0 = min(n_solve, tid * run), j1 = min(n_solve, j0 + run);
    int s = 0;
    for (int j = j0; j < j1; ++j) {
        const int len = als_row_len(rowptr, rows, j);
        s += len > split_len ? (len + split_len - 1) / split_len : 0;
    }
    sums[tid] = s;
    __syncthreads();
    for (int off = 1; off < kPlanBlk; off <<= 1) {                       // inclusive scan of the run sums
        const int v = tid >= off ? sums[tid - off] : 0;
        __syncthreads();
        sums[tid] += v;
        __syncthreads();
    }
    int o = sums[tid] - s;
    for (int j = j0; j < j1; ++j) {
        piece_off[j] = o;
        const int len = als_row_len(rowptr, rows, j);
        o += len > split_len ? (len + split_len - 1) / split_len : 0;
    }
    if (tid == kPlanBlk - 1) piece_off[n_solve] = sums[kPlanBlk - 1];
}

// ------------------------------------------------------------------------------------------------ the normal equations of one run of entries
template <int D>
struct als_cfg {
    static constexpr int NT = D / 16, NP = NT * (NT + 1) / 2, PW = (NP + kWaves - 1) / kWaves, LD = D + 16, Q = D / 4;
    static constexpr int FSTEP = kBlk / Q, PF = kStage / FSTEP, NPART = kBlk / D;
    // the staging image: two stages of 64 gathered rows, their weights, and the b partials of the thread groups
    static constexpr size_t tile_bytes = sizeof(float) * 2 * kStage * LD, wts_bytes = sizeof(float) * 2 * kStage, bpart_bytes = sizeof(double) * kBlk;
    static constexpr size_t stage_bytes = tile_bytes + wts_bytes + bpart_bytes;
    // the solve image: packed lower triangle, the b row, the untouched diagonal, the pivots' reciprocals
    static constexpr size_t solve_bytes = sizeof(double) * ((size_t)D * (D + 1) / 2 + 3 * D);
    static constexpr size_t smem_bytes = stage_bytes > solve_bytes ? stage_bytes : solve_bytes;
    static constexpr size_t piece_bytes = sizeof(float) * NP * 256 + sizeof(double) * D;     // one piece's partial: fp32 tiles, double b
};

// wave wv's k-th tile pair: p = wv + 4 k in the row-major list of the lower triangle (ti >= tj); false past the list's end
__device__ __forceinline__ bool als_pair(int p, int np, int &ti, int &tj) {
    ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= p) ++ti;
    tj = p - ti * (ti + 1) / 2;
    return p < np;
}

// The entries [lo, hi) of the CSR (hi > lo): sv[k][reg] = the wave's tiles of S = sum w y y^T (element (16 ti + 4 g + reg, 16 tj + c) of tile k), and
// bv = element tid of b = sum beta(w) y on the threads tid < D.  Ends with the workgroup synchronised and the staging image free.  RULE is the target
// rule: 0 ('stored') beta(w) = 1 + alpha w, 1 ('relaxed') beta(w) = (1 + alpha) w -- the same double at w = 1, nothing at w = 0.
template <int D, int RULE = 0>
__device__ __forceinline__ void als_accumulate(const float *__restrict__ Y, const int32_t *__restrict__ col, const float *__restrict__ val, int lo, int hi,
                                               double alpha, unsigned char *smem, double (&sv)[als_cfg<D>::PW][4], double &bv) {
#pragma clang fp contract(off)
    typedef als_cfg<D> cfg;
    constexpr int LD = cfg::LD, PW = cfg::PW, PF = cfg::PF, FSTEP = cfg::FSTEP, Q = cfg::Q, NPART = cfg::NPART;
    float *tile = reinterpret_cast<float *>(smem);
    float *wts = reinterpret_cast<float *>(smem + cfg::tile_bytes);
    double *bpart = reinterpret_cast<double *>(smem + cfg::tile_bytes + cfg::wts_bytes);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    int oa[PW], ob[PW];
    bool live[PW];
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        int ti, tj;
        live[k] = als_pair(wv + kWaves * k, cfg::NP, ti, tj);
        oa[k] = live[k] ? 16 * ti + c : c;
        ob[k] = live[k] ? 16 * tj + c : c;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) sv[k][reg] = 0.0;
    }
    const int frow = tid / Q, fq = (tid % Q) * 4;
    const int bcol = tid % D, bpartid = tid / D;
    double bacc = 0.0;
    f32x4v pre[PF];
    float pre_w = 0.f;
    const int nst = (hi - lo + kStage - 1) / kStage;
#define ALS_FETCH(ST)                                                                                                              \
    do {                                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < PF; ++i) {                                                                           \
            const int e = lo + (ST) * kStage + frow + i * FSTEP;                                                                   \
            const int cc = col[min(e, hi - 1)];                                    /* clamped; entries past hi become zero rows */ \
            const f32x4v v = *reinterpret_cast<const f32x4v *>(Y + (size_t)cc * D + fq);                                           \
            pre[i] = e < hi ? v : f32x4v{0.f, 0.f, 0.f, 0.f};                                                                      \
        }                                                                                                                          \
        if (tid < kStage) {                                                                                                        \
            const int e = lo + (ST) * kStage + tid;                                                                                \
            pre_w = e < hi ? (val ? val[e] : 1.f) : 0.f;                                                                           \
        }                                                                                                                          \
    } while (0)
#define ALS_STASH(BUF)                                                                                                             \
    do {                                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < PF; ++i)                                                                             \
            *reinterpret_cast<f32x4v *>(&tile[(BUF) * kStage * LD + (frow + i * FSTEP) * LD + fq]) = pre[i];                       \
        if (tid < kStage) wts[(BUF) * kStage + tid] = pre_w;                                                                       \
    } while (0)
    ALS_FETCH(0);
    ALS_STASH(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) ALS_FETCH(st + 1);
        const float *T = tile + buf * kStage * LD;
        const float *W = wts + buf * kStage;
        f32x4v acc[PW];
#pragma unroll
        for (int k = 0; k < PW; ++k) acc[k] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int kk = 0; kk < kStage / 4; ++kk) {
            const float *row = T + (kk * 4 + g) * LD;
            const float w = W[kk * 4 + g];
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                if (!live[k]) continue;                                  // wave-uniform
                acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(w * row[oa[k]], row[ob[k]], acc[k], 0, 0, 0);
            }
        }
#pragma unroll
        for (int k = 0; k < PW; ++k)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) sv[k][reg] += (double)acc[k][reg];
        for (int r = bpartid; r < kStage; r += NPART)
            bacc += (RULE == 0 ? 1.0 + alpha * (double)W[r] : (1.0 + alpha) * (double)W[r]) * (double)T[r * LD + bcol];
        if (st + 1 < nst) ALS_STASH(buf ^ 1);
        __syncthreads();
    }
#undef ALS_FETCH
#undef ALS_STASH
    bpart[tid] = bacc;                                                   // [NPART][D]: tid = part * D + column
    __syncthreads();
    bv = 0.0;
    if (tid < D) {
#pragma unroll
        for (int p = 0; p < NPART; ++p) bv += bpart[p * D + tid];
    }
    __syncthreads();
}

// One workgroup per piece of a split row: the piece's tiles (fp32, [pair][lane][reg]) and b (double).
template <int D, int RULE = 0>
__global__ __launch_bounds__(kBlk) void als_piece_kernel(const float *__restrict__ Y, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                          const float *__restrict__ val, const int32_t *__restrict__ rows, int n_solve, int split_len,
                                                          int max_pieces, double alpha, const int32_t *__restrict__ piece_off, unsigned char *__restrict__ parts) {
    typedef als_cfg<D> cfg;
    __shared__ __attribute__((aligned(16))) unsigned char smem[cfg::stage_bytes];
    const int p = blockIdx.x;
    if (p >= piece_off[n_solve] || p >= max_pieces) return;
    int a = 0, b = n_solve + 1;                                          // the first index whose offset exceeds p; the row is the one before it
    while (a < b) {
        const int m = (a + b) >> 1;
        if (piece_off[m] > p) b = m; else a = m + 1;
    }
    const int j = a - 1;
    if (piece_off[j + 1] > max_pieces) return;                           // a row whose pieces do not all fit the workspace is solved unsplit
    const int r = rows ? rows[j] : j;
    const int lo = rowptr[r] + (p - piece_off[j]) * split_len, hi = min(rowptr[r + 1], lo + split_len);
    double sv[cfg::PW][4], bv;
    als_accumulate<D, RULE>(Y, col, val, lo, hi, alpha, smem, sv, bv);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float *pt = reinterpret_cast<float *>(parts + (size_t)p * cfg::piece_bytes);
    double *pb = reinterpret_cast<double *>(parts + (size_t)p * cfg::piece_bytes + sizeof(float) * cfg::NP * 256);
#pragma unroll
    for (int k = 0; k < cfg::PW; ++k) {
        const int pr = wv + kWaves * k;
        if (pr >= cfg::NP) continue;
        *reinterpret_cast<f32x4v *>(pt + (size_t)pr * 256 + lane * 4) = f32x4v{(float)sv[k][0], (float)sv[k][1], (float)sv[k][2], (float)sv[k][3]};
    }
    if (tid < D) pb[tid] = bv;
}

__device__ __forceinline__ double als_readlane(double v, int src) {      // src wave-uniform
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src), lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    return __hiloint2double(hi, lo);
}

// One workgroup per listed row: (S, b) from the row's entries or from its pieces, A = G + alpha S + lambda I in LDS, Cholesky, the two substitutions.
// ADJ: the row adjoint z_r = A_r^-1 g_r -- the same A_r, with row j of gX travelling where b_r travels; X then receives z.
template <int D, int RULE = 0, bool ADJ = false>
__global__ __launch_bounds__(kBlk) void als_row_kernel(const float *__restrict__ Y, const double *__restrict__ G, const int32_t *__restrict__ rowptr,
                                                        const int32_t *__restrict__ col, const float *__restrict__ val, const int32_t *__restrict__ rows,
                                                        int n_solve, int max_pieces, double alpha, double lambda, const int32_t *__restrict__ piece_off,
                                                        const unsigned char *__restrict__ parts, float *__restrict__ X, const float *__restrict__ gX) {
    typedef als_cfg<D> cfg;
    constexpr int PW = cfg::PW, TPR = kBlk / D;
    __shared__ __attribute__((aligned(16))) unsigned char smem[cfg::smem_bytes];
    const int j = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r = rows ? rows[j] : j;
    const int lo = rowptr[r], hi = rowptr[r + 1];
    float *xout = X + (size_t)j * D;
    if (hi <= lo) {                                                      // workgroup-uniform: an empty row is exactly 0
        if (tid < D) xout[tid] = 0.f;
        return;
    }
    double sv[PW][4], bv;
    const int p0 = piece_off[j], p1 = piece_off[j + 1];
    if (p1 > p0 && p1 <= max_pieces) {                                   // workgroup-uniform: the pieces in piece order, in double
#pragma unroll
        for (int k = 0; k < PW; ++k)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) sv[k][reg] = 0.0;
        bv = 0.0;
        for (int p = p0; p < p1; ++p) {
            const float *pt = reinterpret_cast<const float *>(parts + (size_t)p * cfg::piece_bytes);
            const double *pb = reinterpret_cast<const double *>(parts + (size_t)p * cfg::piece_bytes + sizeof(float) * cfg::NP * 256);
#pragma unroll
            for (int k = 0; k < PW; ++k) {
                const int pr = wv + kWaves * k;
                if (pr >= cfg::NP) continue;
                const f32x4v v = *reinterpret_cast<const f32x4v *>(pt + (size_t)pr * 256 + lane * 4);
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) sv[k][reg] += (double)v[reg];
            }
            if (tid < D) bv += pb[tid];
        }
    } else {
        als_accumulate<D, RULE>(Y, col, val, lo, hi, alpha, smem, sv, bv);
    }
    if (ADJ) bv = tid < D ? (double)gX[(size_t)j * D + tid] : 0.0;
    // the solve image (the staging image is free: als_accumulate ends synchronised)
    double *Lp = reinterpret_cast<double *>(smem);                       // packed lower triangle: (i, k) at i (i + 1) / 2 + k
    double *zb = Lp + (size_t)D * (D + 1) / 2;                            // the b row, L^-1 b once the factorisation is through
    double *dg = zb + D;                                                  // A's diagonal, untouched
    double *inv = dg + D;                                                 // 1 / L[k][k]
#pragma unroll
    for (int k = 0; k < PW; ++k) {
        int ti, tj;
        if (!als_pair(wv + kWaves * k, cfg::NP, ti, tj)) continue;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int i = 16 * ti + 4 * g + reg, jj = 16 * tj + c;
            if (jj > i) continue;                                        // the upper half of a diagonal tile
            double a = G[(size_t)i * D + jj] + alpha * sv[k][reg];
            if (i == jj) { a += lambda; dg[i] = a; }
            Lp[i * (i + 1) / 2 + jj] = a;
        }
    }
    if (tid < D) zb[tid] = bv;
    __syncthreads();
    // column 0: no sum to subtract
    {
        const double a00 = dg[0], ip = rsqrt(a00);
        if (tid == 0) { Lp[0] = a00 * ip; inv[0] = ip; zb[0] = zb[0] * ip; }
        else if (tid < D) Lp[tid * (tid + 1) / 2] = Lp[tid * (tid + 1) / 2] * ip;
    }
    __syncthreads();
    // columns 1 .. D - 1 (Cholesky-Crout): TPR threads per row split the sum over k < col, every group also sums the pivot row's squares (its
    // operand is loaded anyway), so the pivot is known to every group after the same additions and one barrier per column is enough.  Slot 0's
    // row is finished after column 0: from column 1 on it carries the b row.
    const int slot = tid / TPR, h = tid % TPR;
    for (int cj = 1; cj < D; ++cj) {
        const bool brow = slot == 0, own = brow || slot >= cj;
        const double *Lj = Lp + cj * (cj + 1) / 2;
        double *Li = brow ? zb : Lp + (own ? slot : cj) * ((own ? slot : cj) + 1) / 2;
        double si = 0.0, sp = 0.0;
        int k = h;
        for (; k + 3 * TPR < cj; k += 4 * TPR) {                        // four operand pairs in flight, added in ascending k all the same
            const double a0 = Lj[k], a1 = Lj[k + TPR], a2 = Lj[k + 2 * TPR], a3 = Lj[k + 3 * TPR];
            const double b0 = Li[k], b1 = Li[k + TPR], b2 = Li[k + 2 * TPR], b3 = Li[k + 3 * TPR];
            si += b0 * a0; sp += a0 * a0;
            si += b1 * a1; sp += a1 * a1;
            si += b2 * a2; sp += a2 * a2;
            si += b3 * a3; sp += a3 * a3;
        }
        for (; k < cj; k += TPR) {
            const double ljk = Lj[k];
            si += Li[k] * ljk;
            sp += ljk * ljk;
        }
#pragma unroll
        for (int off = 1; off < TPR; off <<= 1) { si += __shfl_xor(si, off); sp += __shfl_xor(sp, off); }
        const double piv = dg[cj] - sp, ip = rsqrt(piv);               // the pivot is piv * ip = sqrt(piv); the column is scaled by 1 / sqrt(piv)
        const double v = (!brow && slot == cj) ? piv * ip : (Li[cj] - si) * ip;
        if (own && h == 0) {
            Li[cj] = v;
            if (!brow && slot == cj) inv[cj] = ip;
        }
        __syncthreads();
    }
    // L^T x = z in wave 0: lane l keeps elements l and l + 64; x_j leaves by readlane, the lanes below j take it out of their elements
    if (wv != 0) return;
    double z0 = lane < D ? zb[lane] : 0.0, z1 = (D > 64) ? zb[lane + 64 < D ? lane + 64 : 0] : 0.0;
    for (int cj = D - 1; cj >= 0; --cj) {
        const double *Lj = Lp + cj * (cj + 1) / 2;
        const double xj = als_readlane(cj >= 64 ? z1 : z0, cj & 63) * inv[cj];
        if (lane == (cj & 63)) { if (cj >= 64) z1 = xj; else z0 = xj; }
        if (lane < cj) z0 -= Lj[lane] * xj;
        if (D > 64 && lane + 64 < cj) z1 -= Lj[lane + 64] * xj;
    }
    if (lane < D) xout[lane] = (float)z0;
    if (D > 64) xout[lane + 64] = (float)z1;
}

// ------------------------------------------------------------------------------------------------ the objective
// term [u] = x_u^T G x_u + sum_{i in P_u} ((1 + alpha w)(1 - s)^2 - s^2) + lambda |x_u|^2, one wave per row, in double; the lanes' shares are folded
// by a fixed butterfly.
template <int D>
__global__ __launch_bounds__(kBlk) void als_obj_rows_kernel(const float *__restrict__ X, int n_rows, const float *__restrict__ Y, const double *__restrict__ G,
                                                             const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                                             double alpha, double lambda, double *__restrict__ term) {
    __shared__ double xs[kWaves][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, u_ = blockIdx.x * kWaves + wv;
    const bool act = u_ < n_rows;
    const int u = act ? u_ : n_rows - 1;                                 // a wave past the end repeats the last row and writes nothing
    for (int i = lane; i < D; i += 64) xs[wv][i] = (double)X[(size_t)u * D + i];
    __syncthreads();
    const double *x = xs[wv];
    double t = 0.0;
    for (int i = lane; i < D; i += 64) {
        double gi = 0.0;
#pragma unroll 4
        for (int k = 0; k < D; ++k) gi += G[(size_t)k * D + i] * x[k];
        t += x[i] * gi + lambda * x[i] * x[i];
    }
    const int lo = rowptr[u], hi = rowptr[u + 1];
    for (int e = lo + lane; e < hi; e += 64) {
        const float *y = Y + (size_t)col[e] * D;
        double s = 0.0;
#pragma unroll 2
        for (int k = 0; k < D; k += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(y + k);
            s += x[k] * (double)v.x; s += x[k + 1] * (double)v.y; s += x[k + 2] * (double)v.z; s += x[k + 3] * (double)v.w;
        }
        const double w = val ? (double)val[e] : 1.0;
        t += (1.0 + alpha * w) * (1.0 - s) * (1.0 - s) - s * s;
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) t += __shfl_xor(t, off);
    if (lane == 0 && act) term[u] = t;
}

// out [part] = scale * the sum of squares of the part's span of v, in double
__global__ __launch_bounds__(kBlk) void als_sumsq_kernel(const float *__restrict__ v, long long n, long long span, double scale, double *__restrict__ out) {
    __shared__ double red[kBlk];
    const long long b = (long long)blockIdx.x * span, e = b + span < n ? b + span : n;
    double s = 0.0;
    for (long long i = b + threadIdx.x; i < e; i += kBlk) s += (double)v[i] * (double)v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = kBlk / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = scale * red[0];
}

// out [0] = the sum of v [0, n): each thread a contiguous run, the runs by a fixed tree
__global__ __launch_bounds__(kBlk) void als_fold_kernel(const double *__restrict__ v, long long n, double *__restrict__ out) {
    __shared__ double red[kBlk];
    const long long run = (n + kBlk - 1) / kBlk, b = run * threadIdx.x, e = b + run < n ? b + run : n;
    double s = 0.0;
    for (long long i = b; i < e; ++i) s += v[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = kBlk / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ------------------------------------------------------------------------------------------------ the adjoint of the row solve
// Given g_r = dL/dx_r and z_r = A_r^-1 g_r (als_row_kernel<D, 0, true>), with s = x_r . y_i, t = z_r . y_i, beta(w) = b0 + b1 w and C = sum_r z_r x_r^T:
//     dL/dw_ri = t (b1 - alpha s)
//     dL/dy_i  = sum_{r with i} [ (beta(w_ri) - alpha w_ri s) z_r - alpha w_ri t x_r ]  -  y_i (C + C^T)
// Entry pass: coef [e] = (beta - alpha w s, -alpha w t) and dval [e], one wave per row, the dots in double as in als_obj_rows_kernel.
template <int D>
__global__ __launch_bounds__(kBlk) void alsgrad_entry_kernel(const float *__restrict__ X, const float *__restrict__ Z, int n_rows, const float *__restrict__ Y,
                                                              const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                                              double alpha, double b0, double b1, double2 *__restrict__ coef, float *__restrict__ dval) {
    __shared__ double xs[kWaves][D], zs[kWaves][D];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, u_ = blockIdx.x * kWaves + wv;
    const bool act = u_ < n_rows;
    const int u = act ? u_ : n_rows - 1;                                 // a wave past the end loads the last row and writes nothing
    for (int i = lane; i < D; i += 64) { xs[wv][i] = (double)X[(size_t)u * D + i]; zs[wv][i] = (double)Z[(size_t)u * D + i]; }
    __syncthreads();
    const double *x = xs[wv], *z = zs[wv];
    const int lo = rowptr[u], hi = act ? rowptr[u + 1] : lo;
    for (int e = lo + lane; e < hi; e += 64) {
        const float *y = Y + (size_t)col[e] * D;
        double s = 0.0, t = 0.0;
#pragma unroll 2
        for (int k = 0; k < D; k += 4) {
            const float4 v = *reinterpret_cast<const float4 *>(y + k);
            s += x[k] * (double)v.x; s += x[k + 1] * (double)v.y; s += x[k + 2] * (double)v.z; s += x[k + 3] * (double)v.w;
            t += z[k] * (double)v.x; t += z[k + 1] * (double)v.y; t += z[k + 2] * (double)v.z; t += z[k + 3] * (double)v.w;
        }
        const double w = val ? (double)val[e] : 1.0;
        coef[e] = make_double2((b0 + b1 * w) - alpha * w * s, -(alpha * w * t));
        if (dval) dval[e] = (float)(t * (b1 - alpha * s));
    }
}

// part [span][D * D] = sum over the span's rows, ascending, of z x^T in double: als_gram_partial_kernel with two tables.
template <int D>
__global__ __launch_bounds__(kBlk) void alsgrad_xgram_partial_kernel(const float *__restrict__ Z, const float *__restrict__ X, int n, int span,
                                                                      double *__restrict__ part) {
    constexpr int R = D / 16, Q = D / 4;
    __shared__ float tz[kGramStage * D], tx_[kGramStage * D];
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int r_begin = blockIdx.x * span, r_end = min(n, r_begin + span);
    double acc[R][R];
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) acc[a][b] = 0.0;
    for (int r0 = r_begin; r0 < r_end; r0 += kGramStage) {
        for (int idx = tid; idx < kGramStage * Q; idx += kBlk) {
            const int row = idx / Q, q = (idx % Q) * 4;
            float4 vz = make_float4(0.f, 0.f, 0.f, 0.f), vx = vz;                  // rows past the span add exact zeros
            if (r0 + row < r_end) {
                vz = *reinterpret_cast<const float4 *>(Z + (size_t)(r0 + row) * D + q);
                vx = *reinterpret_cast<const float4 *>(X + (size_t)(r0 + row) * D + q);
            }
            *reinterpret_cast<float4 *>(&tz[row * D + q]) = vz;
            *reinterpret_cast<float4 *>(&tx_[row * D + q]) = vx;
        }
        __syncthreads();
        for (int rr = 0; rr < kGramStage; ++rr) {
            double za[R], xb[R];
#pragma unroll
            for (int a = 0; a < R; ++a) { za[a] = (double)tz[rr * D + ty + 16 * a]; xb[a] = (double)tx_[rr * D + tx + 16 * a]; }
#pragma unroll
            for (int a = 0; a < R; ++a)
#pragma unroll
                for (int b = 0; b < R; ++b) acc[a][b] += za[a] * xb[b];
        }
        __syncthreads();
    }
    double *out = part + (size_t)blockIdx.x * D * D;
#pragma unroll
    for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) out[(ty + 16 * a) * D + tx + 16 * b] = acc[a][b];
}

// Cs [i][j] = C [i][j] + C [j][i], each C element the spans' partials in span order: symmetric bit for bit.
__global__ __launch_bounds__(kBlk) void alsgrad_xgram_fold_kernel(const double *__restrict__ part, int ns, int d, double *__restrict__ Cs) {
    const int e = blockIdx.x * kBlk + threadIdx.x, dd = d * d;
    if (e >= dd) return;
    const int et = (e % d) * d + e / d;
    double v = part[e], vt = part[et];
    for (int s = 1; s < ns; ++s) { v += part[(size_t)s * dd + e]; vt += part[(size_t)s * dd + et]; }
    Cs[e] = v + vt;
}

// Element tid (on the threads tid < D) of sum_e (coef[tperm[e]].x z_row + coef[tperm[e]].y x_row) over the entries [lo, hi) of the transposed order:
// thread group g of the kBlk / D groups takes the entries lo + g, lo + g + groups, ... in ascending order, the groups are added in group order.
template <int D>
__device__ __forceinline__ double alsgrad_col_sum(const float *__restrict__ Z, const float *__restrict__ X, const int32_t *__restrict__ trow,
                                                  const int32_t *__restrict__ tperm, const double2 *__restrict__ coef, int lo, int hi, double *red) {
    constexpr int NPART = kBlk / D;
    const int tid = threadIdx.x, k = tid % D, part = tid / D;
    double acc = 0.0;
#pragma unroll 4
    for (int e = lo + part; e < hi; e += NPART) {
        const size_t r = (size_t)trow[e] * D + k;
        const double2 c = coef[tperm[e]];
        acc += c.x * (double)Z[r] + c.y * (double)X[r];
    }
    red[tid] = acc;
    __syncthreads();
    double v = 0.0;
    if (tid < D) {
#pragma unroll
        for (int p = 0; p < NPART; ++p) v += red[p * D + tid];
    }
    __syncthreads();
    return v;
}

// One workgroup per piece of a split column: its partial sum, D doubles.
template <int D>
__global__ __launch_bounds__(kBlk) void alsgrad_colpiece_kernel(const float *__restrict__ Z, const float *__restrict__ X, const int32_t *__restrict__ tptr,
                                                                 const int32_t *__restrict__ trow, const int32_t *__restrict__ tperm,
                                                                 const double2 *__restrict__ coef, int n, int split_len, int max_pieces,
                                                                 const int32_t *__restrict__ piece_off, double *__restrict__ cparts) {
    __shared__ double red[kBlk];
    const int p = blockIdx.x;
    if (p >= piece_off[n] || p >= max_pieces) return;
    int a = 0, b = n + 1;                                                // the first index whose offset exceeds p; the column is the one before it
    while (a < b) {
        const int m = (a + b) >> 1;
        if (piece_off[m] > p) b = m; else a = m + 1;
    }
    const int i = a - 1;
    if (piece_off[i + 1] > max_pieces) return;                           // a column whose pieces do not all fit the workspace is summed unsplit
    const int lo = tptr[i] + (p - piece_off[i]) * split_len, hi = min(tptr[i + 1], lo + split_len);
    const double v = alsgrad_col_sum<D>(Z, X, trow, tperm, coef, lo, hi, red);
    if ((int)threadIdx.x < D) cparts[(size_t)p * D + threadIdx.x] = v;
}

// One workgroup per row i of Y: dY_i = the column's sum (from its entries, or from its pieces in piece order) - y_i Cs.
template <int D>
__global__ __launch_bounds__(kBlk) void alsgrad_col_kernel(const float *__restrict__ Y, const float *__restrict__ Z, const float *__restrict__ X,
                                                            const int32_t *__restrict__ tptr, const int32_t *__restrict__ trow, const int32_t *__restrict__ tperm,
                                                            const double2 *__restrict__ coef, const double *__restrict__ Cs, int max_pieces,
                                                            const int32_t *__restrict__ piece_off, const double *__restrict__ cparts, float *__restrict__ dY) {
    __shared__ double red[kBlk];
    __shared__ double ys[D];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int lo = tptr[i], hi = tptr[i + 1];
    const int p0 = piece_off[i], p1 = piece_off[i + 1];
    if (tid < D) ys[tid] = (double)Y[(size_t)i * D + tid];
    double v = 0.0;
    if (p1 > p0 && p1 <= max_pieces) {                                   // workgroup-uniform
        if (tid < D)
            for (int p = p0; p < p1; ++p) v += cparts[(size_t)p * D + tid];
    } else if (hi > lo) {
        v = alsgrad_col_sum<D>(Z, X, trow, tperm, coef, lo, hi, red);
    }
    __syncthreads();
    if (tid >= D) return;
    double g = 0.0;
#pragma unroll 4
    for (int j = 0; j < D; ++j) g += ys[j] * Cs[(size_t)j * D + tid];
    dY[(size_t)i * D + tid] = (float)(v - g);
}

// ------------------------------------------------------------------------------------------------ host side
bool als_width(int64_t d) { return d == 16 || d == 32 || d == 64 || d == 128; }
bool als_rows_ok(int64_t n) { return n > 0 && n <= 0x7fffffffll / 128; }

size_t als_piece_bytes(int64_t d) {
    const size_t nt = (size_t)d / 16;
    return sizeof(float) * (nt * (nt + 1) / 2) * 256 + sizeof(double) * (size_t)d;
}

// an upper bound of the pieces of the listed rows: a split row is longer than split_len, so there are at most nnz / split_len of them, and
// sum ceil(len / split_len) <= nnz / split_len + their number
int64_t als_max_pieces(int64_t n_solve, int64_t nnz_listed, int64_t split_len) {
    const int64_t q = nnz_listed / split_len;
    return q + (q < n_solve ? q : n_solve);
}

int64_t als_split(int64_t split_len) { return split_len > 0 ? split_len : kDefaultSplit; }

template <int D, int RULE = 0, bool ADJ = false>
int als_solve_run(const float *Y, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *rows, int64_t n_solve,
                  int64_t nnz_listed, double alpha, double lambda, int64_t split_len, float *X, char *ws, hipStream_t st, const float *gX = nullptr) {
    const int64_t mp = als_max_pieces(n_solve, nnz_listed, split_len);
    int32_t *piece_off = (int32_t *)ws;
    unsigned char *parts = (unsigned char *)(ws + up16(sizeof(int32_t) * (size_t)(n_solve + 1)));
    hipLaunchKernelGGL(als_plan_kernel, dim3(1), dim3(kPlanBlk), 0, st, rowptr, rows, (int)n_solve, (int)split_len, piece_off);
    ARL_LAUNCH_CHECK();
    if (mp > 0) {
        hipLaunchKernelGGL((als_piece_kernel<D, RULE>), dim3((unsigned)mp), dim3(kBlk), 0, st, Y, rowptr, col, val, rows, (int)n_solve, (int)split_len, (int)mp, alpha,
                           (const int32_t *)piece_off, parts);
        ARL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((als_row_kernel<D, RULE, ADJ>), dim3((unsigned)n_solve), dim3(kBlk), 0, st, Y, G, rowptr, col, val, rows, (int)n_solve, (int)mp, alpha,
                       lambda, (const int32_t *)piece_off, (const unsigned char *)parts, X, gX);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t alsgrad_col_split(int64_t col_split_len) { return col_split_len > 0 ? col_split_len : kDefaultColSplit; }

// the adjoint's workspace: the row solve's (piece plan, pieces), z, the entries' coefficients, the cross-Gram's partials and C + C^T, the columns' piece
// plan and pieces
struct alsgrad_ws { size_t solve, z, coef, xpart, cs, cplan, cparts, total; int64_t max_cpieces; };
alsgrad_ws alsgrad_layout(int64_t n, int64_t n_rows, int64_t nnz, int64_t d, int64_t split_len, int64_t col_split_len) {
    alsgrad_ws w;
    size_t o = 0;
    w.solve = o; o += up16(up16(sizeof(int32_t) * (size_t)(n_rows + 1)) + (size_t)als_max_pieces(n_rows, nnz, split_len) * als_piece_bytes(d));
    w.z = o;     o += up16(sizeof(float) * (size_t)n_rows * (size_t)d);
    w.coef = o;  o += up16(sizeof(double2) * (size_t)nnz);
    w.xpart = o; o += up16(sizeof(double) * (size_t)gram_splits(n_rows).ns * (size_t)d * (size_t)d);
    w.cs = o;    o += up16(sizeof(double) * (size_t)d * (size_t)d);
    w.cplan = o; o += up16(sizeof(int32_t) * (size_t)(n + 1));
    w.max_cpieces = als_max_pieces(n, nnz, col_split_len);
    w.cparts = o; o += up16(sizeof(double) * (size_t)w.max_cpieces * (size_t)d);
    w.total = o;
    return w;
}

template <int D>
int alsgrad_run(const float *Y, int64_t n, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows, int64_t nnz,
                const float *X, const float *gX, const int32_t *tptr, const int32_t *trow, const int32_t *tperm, double alpha, double lambda, double b0,
                double b1, int64_t split_len, int64_t col_split_len, float *dY, float *dval, char *ws, hipStream_t st) {
    const alsgrad_ws w = alsgrad_layout(n, n_rows, nnz, D, split_len, col_split_len);
    float *Z = (float *)(ws + w.z);
    double2 *coef = (double2 *)(ws + w.coef);
    double *xpart = (double *)(ws + w.xpart), *Cs = (double *)(ws + w.cs), *cparts = (double *)(ws + w.cparts);
    int32_t *cplan = (int32_t *)(ws + w.cplan);
    // z_r = A_r^-1 g_r: the forward's launches with g as the extra row
    const int rc = als_solve_run<D, 0, true>(Y, G, rowptr, col, val, nullptr, n_rows, nnz, alpha, lambda, split_len, Z, ws + w.solve, st, gX);
    if (rc != ARL_OK) return rc;
    hipLaunchKernelGGL((alsgrad_entry_kernel<D>), dim3((unsigned)((n_rows + kWaves - 1) / kWaves)), dim3(kBlk), 0, st, X, (const float *)Z, (int)n_rows, Y, rowptr,
                       col, val, alpha, b0, b1, coef, dval);
    ARL_LAUNCH_CHECK();
    const gram_split gs = gram_splits(n_rows);
    hipLaunchKernelGGL((alsgrad_xgram_partial_kernel<D>), dim3((unsigned)gs.ns), dim3(kBlk), 0, st, (const float *)Z, X, (int)n_rows, gs.span, xpart);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(alsgrad_xgram_fold_kernel, dim3((unsigned)((D * D + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const double *)xpart, gs.ns, D, Cs);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(als_plan_kernel, dim3(1), dim3(kPlanBlk), 0, st, tptr, (const int32_t *)nullptr, (int)n, (int)col_split_len, cplan);
    ARL_LAUNCH_CHECK();
    if (w.max_cpieces > 0) {
        hipLaunchKernelGGL((alsgrad_colpiece_kernel<D>), dim3((unsigned)w.max_cpieces), dim3(kBlk), 0, st, (const float *)Z, X, tptr, trow, tperm,
                           (const double2 *)coef, (int)n, (int)col_split_len, (int)w.max_cpieces, (const int32_t *)cplan, cparts);
        ARL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((alsgrad_col_kernel<D>), dim3((unsigned)n), dim3(kBlk), 0, st, Y, (const float *)Z, X, tptr, trow, tperm, (const double2 *)coef,
                       (const double *)Cs, (int)w.max_cpieces, (const int32_t *)cplan, (const double *)cparts, dY);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_als_default_split_len(void) { return kDefaultSplit; }

int64_t arl_als_gram_workspace_bytes(int64_t n, int64_t d) {
    if (!als_width(d) || !als_rows_ok(n)) return 0;
    return (int64_t)(sizeof(double) * (size_t)gram_splits(n).ns * (size_t)d * (size_t)d);
}

int arl_als_gram_f64(const float *Y, int64_t n, int64_t d, double *G, void *workspace, arl_stream_t stream) {
    if (!Y || !G || !workspace) return ARL_E_NULL;
    if (!als_width(d)) return ARL_E_DIM;
    if (n <= 0) return ARL_E_ARG;
    if (!als_rows_ok(n)) return ARL_E_RANGE;
    if (((uintptr_t)Y | (uintptr_t)G | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const gram_split gs = gram_splits(n);
    double *part = (double *)workspace;
#define ALS_GRAM(DD) hipLaunchKernelGGL((als_gram_partial_kernel<DD>), dim3((unsigned)gs.ns), dim3(kBlk), 0, st, Y, (int)n, gs.span, part)
    if (d == 16) ALS_GRAM(16);
    else if (d == 32) ALS_GRAM(32);
    else if (d == 64) ALS_GRAM(64);
    else ALS_GRAM(128);
#undef ALS_GRAM
    ARL_LAUNCH_CHECK();
    const int dd = (int)(d * d);
    hipLaunchKernelGGL(als_gram_fold_kernel, dim3((unsigned)((dd + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const double *)part, gs.ns, dd, G);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_als_solve_rows_workspace_bytes(int64_t n_solve, int64_t nnz_listed, int64_t d, int64_t split_len) {
    if (!als_width(d) || n_solve <= 0 || n_solve > 0x7fffffffll - 1 || nnz_listed < 0 || nnz_listed > 0x7fffffffll) return 0;
    split_len = als_split(split_len);
    return (int64_t)(up16(sizeof(int32_t) * (size_t)(n_solve + 1)) + (size_t)als_max_pieces(n_solve, nnz_listed, split_len) * als_piece_bytes(d));
}

int arl_als_solve_rows_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                           const int32_t *rows, int64_t n_solve, int64_t nnz_listed, double alpha, double lambda, int64_t split_len, float *X, void *workspace,
                           arl_stream_t stream) {
    if (!Y || !G || !rowptr || !col || !X || !workspace) return ARL_E_NULL;
    if (!als_width(d)) return ARL_E_DIM;
    if (n <= 0 || n_rows <= 0 || n_solve <= 0 || nnz_listed < 0 || !(alpha >= 0.0) || !(lambda >= 0.0)) return ARL_E_ARG;
    if (!als_rows_ok(n) || !als_rows_ok(n_solve) || n_rows > 0x7fffffffll - 1 || nnz_listed > 0x7fffffffll) return ARL_E_RANGE;
    if (((uintptr_t)Y | (uintptr_t)G | (uintptr_t)X | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    split_len = als_split(split_len);
    if (split_len > 0x7fffffffll) split_len = 0x7fffffffll;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define ALS_RUN(DD) return als_solve_run<DD>(Y, G, rowptr, col, val, rows, n_solve, nnz_listed, alpha, lambda, split_len, X, ws, st)
    if (d == 16) ALS_RUN(16);
    if (d == 32) ALS_RUN(32);
    if (d == 64) ALS_RUN(64);
    ALS_RUN(128);
#undef ALS_RUN
}

int64_t arl_als_solve_rows_target_workspace_bytes(int64_t n_solve, int64_t nnz_listed, int64_t d, int64_t split_len) {
    return arl_als_solve_rows_workspace_bytes(n_solve, nnz_listed, d, split_len);
}

int arl_als_solve_rows_target_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val,
                                  int64_t n_rows, const int32_t *rows, int64_t n_solve, int64_t nnz_listed, double alpha, double lambda, int32_t target,
                                  int64_t split_len, float *X, void *workspace, arl_stream_t stream) {
    if (target == ARL_ALS_TARGET_STORED)                                 // the same launches: the same bits
        return arl_als_solve_rows_f32(Y, n, d, G, rowptr, col, val, n_rows, rows, n_solve, nnz_listed, alpha, lambda, split_len, X, workspace, stream);
    if (!Y || !G || !rowptr || !col || !X || !workspace) return ARL_E_NULL;
    if (!als_width(d)) return ARL_E_DIM;
    if (target != ARL_ALS_TARGET_RELAXED) return ARL_E_ARG;
    if (n <= 0 || n_rows <= 0 || n_solve <= 0 || nnz_listed < 0 || !(alpha >= 0.0) || !(lambda >= 0.0)) return ARL_E_ARG;
    if (!als_rows_ok(n) || !als_rows_ok(n_solve) || n_rows > 0x7fffffffll - 1 || nnz_listed > 0x7fffffffll) return ARL_E_RANGE;
    if (((uintptr_t)Y | (uintptr_t)G | (uintptr_t)X | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    split_len = als_split(split_len);
    if (split_len > 0x7fffffffll) split_len = 0x7fffffffll;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define ALS_RUN(DD) return als_solve_run<DD, 1>(Y, G, rowptr, col, val, rows, n_solve, nnz_listed, alpha, lambda, split_len, X, ws, st)
    if (d == 16) ALS_RUN(16);
    if (d == 32) ALS_RUN(32);
    if (d == 64) ALS_RUN(64);
    ALS_RUN(128);
#undef ALS_RUN
}

int64_t arl_als_default_col_split_len(void) { return kDefaultColSplit; }

int64_t arl_als_adjoint_workspace_bytes(int64_t n, int64_t n_rows, int64_t nnz, int64_t d, int64_t split_len, int64_t col_split_len) {
    if (!als_width(d) || !als_rows_ok(n) || !als_rows_ok(n_rows) || nnz <= 0 || nnz > 0x7fffffffll) return 0;
    return (int64_t)alsgrad_layout(n, n_rows, nnz, d, als_split(split_len), alsgrad_col_split(col_split_len)).total;
}

int arl_als_adjoint_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                        int64_t nnz, const float *X, const float *gX, const int32_t *tptr, const int32_t *trow, const int32_t *tperm, double alpha,
                        double lambda, int32_t target, int64_t split_len, int64_t col_split_len, float *dY, float *dval, void *workspace,
                        arl_stream_t stream) {
    if (!Y || !G || !rowptr || !col || !X || !gX || !tptr || !trow || !tperm || !dY || !workspace) return ARL_E_NULL;
    if (!als_width(d)) return ARL_E_DIM;
    if (target != ARL_ALS_TARGET_STORED && target != ARL_ALS_TARGET_RELAXED) return ARL_E_ARG;
    if (n <= 0 || n_rows <= 0 || nnz <= 0 || !(alpha >= 0.0) || !(lambda >= 0.0)) return ARL_E_ARG;
    if (!als_rows_ok(n) || !als_rows_ok(n_rows) || nnz > 0x7fffffffll) return ARL_E_RANGE;
    if (((uintptr_t)Y | (uintptr_t)G | (uintptr_t)X | (uintptr_t)gX | (uintptr_t)dY | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    split_len = als_split(split_len);
    col_split_len = alsgrad_col_split(col_split_len);
    if (split_len > 0x7fffffffll) split_len = 0x7fffffffll;
    if (col_split_len > 0x7fffffffll) col_split_len = 0x7fffffffll;
    if (als_max_pieces(n_rows, nnz, split_len) > 0x7fffffffll || als_max_pieces(n, nnz, col_split_len) > 0x7fffffffll) return ARL_E_RANGE;
    const double b0 = target == ARL_ALS_TARGET_STORED ? 1.0 : 0.0, b1 = target == ARL_ALS_TARGET_STORED ? alpha : 1.0 + alpha;
    hipStream_t st = (hipStream_t)stream;
#define ALS_RUN(DD) return alsgrad_run<DD>(Y, n, G, rowptr, col, val, n_rows, nnz, X, gX, tptr, trow, tperm, alpha, lambda, b0, b1, split_len, col_split_len, dY, dval, (char *)workspace, st)
    if (d == 16) ALS_RUN(16);
    if (d == 32) ALS_RUN(32);
    if (d == 64) ALS_RUN(64);
    ALS_RUN(128);
#undef ALS_RUN
}

int64_t arl_als_objective_workspace_bytes(int64_t n_rows, int64_t n, int64_t d) {
    if (!als_width(d) || !als_rows_ok(n) || !als_rows_ok(n_rows)) return 0;
    return (int64_t)(sizeof(double) * ((size_t)n_rows + 2 * kSumParts));
}

int arl_als_objective_f64(const float *X, int64_t n_rows, const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col,
                          const float *val, double alpha, double lambda, double *out, void *workspace, arl_stream_t stream) {
    if (!X || !Y || !G || !rowptr || !col || !out || !workspace) return ARL_E_NULL;
    if (!als_width(d)) return ARL_E_DIM;
    if (n <= 0 || n_rows <= 0) return ARL_E_ARG;
    if (!als_rows_ok(n) || !als_rows_ok(n_rows)) return ARL_E_RANGE;
    if (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)G | (uintptr_t)workspace) & 15 || ((uintptr_t)out & 7)) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    double *term = (double *)workspace;                                  // [n_rows] row terms, then lambda |Y|^2 in kSumParts spans
    const unsigned blocks = (unsigned)((n_rows + kWaves - 1) / kWaves);
#define ALS_OBJ(DD) hipLaunchKernelGGL((als_obj_rows_kernel<DD>), dim3(blocks), dim3(kBlk), 0, st, X, (int)n_rows, Y, G, rowptr, col, val, alpha, lambda, term)
    if (d == 16) ALS_OBJ(16);
    else if (d == 32) ALS_OBJ(32);
    else if (d == 64) ALS_OBJ(64);
    else ALS_OBJ(128);
#undef ALS_OBJ
    ARL_LAUNCH_CHECK();
    const long long ny = (long long)n * d;
    long long parts = (ny + 4095) / 4096;
    if (parts > kSumParts) parts = kSumParts;
    const long long span = (ny + parts - 1) / parts;
    parts = (ny + span - 1) / span;
    hipLaunchKernelGGL(als_sumsq_kernel, dim3((unsigned)parts), dim3(kBlk), 0, st, Y, ny, span, lambda, term + n_rows);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(als_fold_kernel, dim3(1), dim3(kBlk), 0, st, (const double *)term, (long long)n_rows + parts, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

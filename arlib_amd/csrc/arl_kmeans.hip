// arl_kmeans.hip -- Lloyd's k-means for NCL's prototype step (reference recommender/NCL.py:52-73: e_step / run_kmeans) on gfx950, and the greedy
// k-means++ start sklearn gives it (further down).
//
// One iteration is  assign: label[n] = argmax_c (<x_n, c> - 1/2 |c|^2)  (the nearest centroid; |x_n|^2 does not depend on c), then
// update: C[c] = mean of the rows labelled c.  The inertia of an assign pass is  sum_n |x_n|^2 - 2 sum_n best[n].
//
// Rules kept throughout:
//   * the N x k scores are never stored: products run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h): the POINTS
//     are resident, the CENTROIDS and their bias -1/2 |c|^2 are streamed, every lane keeps a running (best, index) over the centroids it sees,
//     the four lanes of a point reduce at the end;
//   * ties go to the LOWER centroid index: a lane meets its centroids in ascending order and replaces its best only on a strict >, the
//     cross-lane reduce prefers the lower index on equal scores;
//   * the running index starts at 0, so a point whose scores are all NaN gets label 0 -- labels index the centroid table, never out of range;
//   * every sum has a fixed order (no float atomics): the bias is a sequential row sum, a cluster's members are walked in ascending row order
//     in chunks of kChunk rows whose partials are folded in chunk order, the inertia sums are double over fixed spans;
//   * a cluster without members keeps its previous centroid bit for bit; the mean is sum / count (a division, not a product with 1 / count).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr int kChunk = 256;                  // member rows per partial sum of the update
constexpr int kSumParts = 1024;              // spans of the double sums
using strm::f32x4v;

// bias[c] = -1/2 |C[c]|^2, one thread per centroid, components in order
__global__ __launch_bounds__(kBlk) void km_bias_kernel(const float *__restrict__ C, int K, int d, float *__restrict__ bias) {
    const int c = blockIdx.x * kBlk + threadIdx.x;
    if (c >= K) return;
    const float4 *row = reinterpret_cast<const float4 *>(C + (size_t)c * d);
    float s = 0.f;
    for (int q = 0; q < d / 4; ++q) {
        const float4 v = row[q];
        s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    bias[c] = -0.5f * s;
}

// labels[n] = the centroid with the largest <x_n, c> + bias[c] (lowest index on a tie, 0 if no score compares), score[n] = that value
template <int D>
__global__ __launch_bounds__(kBlk) void km_assign_kernel(const float *__restrict__ X, int N, const float *__restrict__ Cn, const float *__restrict__ bias, int K,
                                                          int32_t *__restrict__ labels, float *__restrict__ score) {
    __shared__ __attribute__((aligned(16))) float tile[2][strm::kStageFloats<D>];
    __shared__ __attribute__((aligned(16))) float tbias[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    float br[D / 4];
    strm::load_resident<D>(X, r0 + c, N, g, br);
    float best = -INFINITY;
    int bi = 0;
    const int nst = (K + 63) / 64;
    // beside a stage's centroids: their bias, fetched and stashed with them
    strm::stage<D> stg(tid);
    float pre_b = 0.f;
#define KM_FETCH(ST)                                             \
    do {                                                         \
        stg.fetch(Cn, (ST) * 64, K);                             \
        if (tid < 64) pre_b = bias[min((ST) * 64 + tid, K - 1)]; \
    } while (0)
#define KM_STASH(BUF)                          \
    do {                                       \
        stg.stash(tile[BUF]);                  \
        if (tid < 64) tbias[BUF][tid] = pre_b; \
    } while (0)
    KM_FETCH(0); KM_STASH(0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) KM_FETCH(st + 1);
        f32x4v sc[4];                                                    // the stage's four 16-centroid tiles
        strm::scores4<D>(tile[buf], c, g, br, sc);
        // register j of tile sub is centroid st * 64 + sub * 16 + 4 g + j against point r0 + c: ascending in (sub, j), so a strict > keeps the lower index
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int cb = st * 64 + sub * 16 + 4 * g;
            const float4 b4 = *reinterpret_cast<const float4 *>(&tbias[buf][sub * 16 + 4 * g]);
            const float bj[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = sc[sub][j] + bj[j];
                if (cb + j < K && v > best) { best = v; bi = cb + j; }
            }
        }
        if (st + 1 < nst) KM_STASH(buf ^ 1);
        __syncthreads();
    }
#undef KM_FETCH
#undef KM_STASH
    // the four lane groups of a point: the larger score, on equal scores the lower index (both lanes of a pair decide alike)
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {
        const float v2 = __shfl_xor(best, off);
        const int i2 = __shfl_xor(bi, off);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if (g == 0 && r0 + c < N) {
        labels[r0 + c] = bi;
        score[r0 + c] = best;
    }
}

// one workgroup per chunk of a cluster's member list: part[b][:] = sum of X[order[p]] over the chunk's positions p, ascending.
// chunk_ptr[c] = chunks of the clusters before c; workgroups past chunk_ptr[K] have nothing to do.
__global__ __launch_bounds__(kBlk) void km_segsum_kernel(const float *__restrict__ X, int N, int d, const int32_t *__restrict__ order, const int32_t *__restrict__ seg_ptr,
                                                          const int32_t *__restrict__ chunk_ptr, int K, float *__restrict__ part) {
    __shared__ float4 red[kBlk];
    const int b = blockIdx.x;
    if (b >= chunk_ptr[K]) return;
    int lo = 0, hi = K - 1;                       // the last c with chunk_ptr[c] <= b; clusters without chunks share a value and are skipped
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (chunk_ptr[mid] <= b) lo = mid; else hi = mid - 1;
    }
    const int d4 = d >> 2, q = threadIdx.x % d4, rl = threadIdx.x / d4, lanes = kBlk / d4;
    const long long p_begin = (long long)seg_ptr[lo] + (long long)(b - chunk_ptr[lo]) * kChunk;
    long long p_end = p_begin + kChunk;
    if (p_end > seg_ptr[lo + 1]) p_end = seg_ptr[lo + 1];
    if (p_end > N) p_end = N;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long p = (p_begin < 0 ? 0 : p_begin) + rl; p < p_end; p += lanes) {
        const int r = order[p];
        if ((unsigned)r >= (unsigned)N) continue;
        const float4 v = *reinterpret_cast<const float4 *>(X + (size_t)r * d + 4 * q);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
        for (int j = 1; j < lanes; ++j) {
            const float4 v = red[j * d4 + q];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4 *>(part + (size_t)b * d + 4 * q) = s;
    }
}

// C_new[c] = (the cluster's partials in chunk order) / count, or C_prev[c] for a cluster without members
__global__ __launch_bounds__(kBlk) void km_mean_kernel(const float *__restrict__ part, const int32_t *__restrict__ seg_ptr, const int32_t *__restrict__ chunk_ptr, int K, int d,
                                                        const float *__restrict__ C_prev, float *__restrict__ C_new) {
    const int e = blockIdx.x * kBlk + threadIdx.x;
    if (e >= K * d) return;
    const int c = e / d, col = e - c * d;
    const int count = seg_ptr[c + 1] - seg_ptr[c];
    if (count <= 0) { C_new[e] = C_prev[e]; return; }
    float s = 0.f;
    for (int j = chunk_ptr[c]; j < chunk_ptr[c + 1]; ++j) s += part[(size_t)j * d + col];
    C_new[e] = s / (float)count;
}

// part[b] = sum of v (or v^2) over the b-th span in double: a thread's strided elements, then a tree over the workgroup
__global__ __launch_bounds__(kBlk) void km_sum_partial_kernel(const float *__restrict__ v, long long n, long long span, int squared, double *__restrict__ part) {
    __shared__ double red[kBlk];
    const long long begin = (long long)blockIdx.x * span, end = min(n, begin + span);
    double s = 0.0;
    for (long long i = begin + threadIdx.x; i < end; i += kBlk) {
        const double x = (double)v[i];
        s += squared ? x * x : x;
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlk / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBlk) void km_sum_fold_kernel(const double *__restrict__ part, int n_part, double *__restrict__ out) {
    __shared__ double red[kBlk];
    double s = 0.0;
    for (int b = threadIdx.x; b < n_part; b += kBlk) s += part[b];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlk / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = red[0];
}

// ---------------------------------------------------------------------------------------------------------------- greedy k-means++ start
// (sklearn's _kmeans_plusplus with unit weights).  State: closest[n] = squared distance of row n to its nearest chosen centre.
// A step measures every row against T <= 16 candidate rows (dist), then folds the potentials, takes the winner and draws the next candidates (pick).
//   * distances are direct sums of squared differences (no |x|^2 - 2<x,c> + |c|^2: nothing cancels, the error is relative);
//   * a workgroup owns a fixed span of rows (a multiple of kPpRows; at most kPpMaxSpans spans), four lanes share a row, a lane keeps every 4th float4
//     of two rows (one at d = 128) in registers, the candidates sit in LDS; the potentials are double per lane, folded by a fixed shuffle tree and over the four waves in order;
//   * the winner's minima are not copied: the next pass reads them where they lie, through the winner's index on the device;
//   * every id and selector read from device memory is clamped before it addresses anything, and every comparison that finds a row is written so that
//     a NaN leaves an index inside [0, N): ids address X afterwards.
constexpr int kPpLanes = 4;                                   // lanes per row
constexpr int kPpRows = 2 * kBlk / kPpLanes;                  // spans are multiples of the widest workgroup sweep (two rows per lane group)
constexpr int kPpMaxSpans = 1024, kPpMaxT = 16;
constexpr int kPickBlk = 64 * kPpMaxT;                        // one wave per candidate
constexpr int kPickRows = 8;                                  // rows per lane in flight in the walk inside a span

inline int kpp_span(long long N) {
    const long long per = (N + kPpMaxSpans - 1) / kPpMaxSpans;
    return (int)((per + kPpRows - 1) / kPpRows * kPpRows);
}

__device__ inline int kpp_clamp(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }          // an int is never a NaN: always inside [0, n)

// mins[t][n] = min(closest[n], |x_n - x_{id_t}|^2) (closest = +inf without closest_base), part[t][b] = the sum of mins[t] over span b in double.
// TT >= T candidates are computed (the surplus repeats the last one and is not stored); closest = closest_base + sel[0] * N.
template <int D, int TT>
__global__ __launch_bounds__(kBlk, 4) void kpp_dist_kernel(const float *__restrict__ X, int N, int span, const int32_t *__restrict__ cand_ids, int id0, int T,
                                                            const float *__restrict__ closest_base, const int32_t *__restrict__ sel, int n_sel,
                                                            float *__restrict__ mins, double *__restrict__ part, int S) {
    constexpr int Q = D / (4 * kPpLanes), D4 = D / 4, R = D == 128 ? 1 : 2, G = kBlk / kPpLanes;      // R rows per lane group and sweep
    __shared__ float4 cand[TT * D4];
    __shared__ double wred[kPpMaxT][kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, j = tid & (kPpLanes - 1), g = tid / kPpLanes;
    const float4 *X4 = reinterpret_cast<const float4 *>(X);
    for (int i = tid; i < TT * D4; i += kBlk) {
        const int t = min(i / D4, T - 1);
        const int id = kpp_clamp(cand_ids ? cand_ids[t] : id0, N);
        cand[i] = X4[(size_t)id * D4 + (i % D4)];
    }
    const float *closest = nullptr;
    if (closest_base) closest = closest_base + (size_t)kpp_clamp(sel ? sel[0] : 0, n_sel) * N;
    __syncthreads();
    double pot[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) pot[t] = 0.0;
    const int begin = blockIdx.x * span, end = min(N, begin + span);
    for (int r0 = begin + g; r0 < end + g; r0 += R * G) {              // every lane runs every sweep: the shuffles below need the whole wave
        asm volatile("" ::: "memory");                               // the candidates are read from LDS in every sweep: hoisted out of the loop they cost T D / 4 registers
        float4 x[R][Q];
        float cl[R];
#pragma unroll
        for (int i = 0; i < R; ++i) {
            const int r = r0 + i * G;
#pragma unroll
            for (int q = 0; q < Q; ++q) x[i][q] = r < end ? X4[(size_t)r * D4 + q * kPpLanes + j] : make_float4(0.f, 0.f, 0.f, 0.f);
            cl[i] = closest && j == 0 && r < end ? closest[r] : INFINITY;
        }
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            float s[R];
#pragma unroll
            for (int i = 0; i < R; ++i) s[i] = 0.f;
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const float4 c = cand[t * D4 + q * kPpLanes + j];
#pragma unroll
                for (int i = 0; i < R; ++i) {
                    float e;
                    e = x[i][q].x - c.x; s[i] = fmaf(e, e, s[i]);
                    e = x[i][q].y - c.y; s[i] = fmaf(e, e, s[i]);
                    e = x[i][q].z - c.z; s[i] = fmaf(e, e, s[i]);
                    e = x[i][q].w - c.w; s[i] = fmaf(e, e, s[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < R; ++i) {
                s[i] += __shfl_xor(s[i], 1);
                s[i] += __shfl_xor(s[i], 2);
                const int r = r0 + i * G;
                if (t < T && j == 0 && r < end) {
                    const float m = cl[i] <= s[i] ? cl[i] : s[i];          // numpy's minimum: a NaN distance stays a NaN
                    mins[(size_t)t * N + r] = m;
                    pot[t] += (double)m;
                }
            }
        }
    }
#pragma unroll
    for (int t = 0; t < TT; ++t) {
        if (t < T) {
            double v = pot[t];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) wred[t][wv] = v;
        }
    }
    __syncthreads();
    if (tid < T) part[(size_t)tid * S + blockIdx.x] = ((wred[tid][0] + wred[tid][1]) + wred[tid][2]) + wred[tid][3];
}

__device__ inline double kpp_wave_scan(double v, int lane) {                      // inclusive, over the 64 lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double o = __shfl_up(v, off);
        if (lane >= off) v += o;
    }
    return v;
}

// One workgroup, wave t for candidate t.  pot_t = the fold of part[t] (a lane's strided spans, then a shuffle tree); the winner is the lowest t with the
// smallest pot_t (a NaN never compares smaller: the winner stays inside [0, T)); sel_out = that t, index_out = its row.  With T_next > 0 wave j draws
// next_ids[j]: the first row whose inclusive running sum of the winner's minima reaches u[j] * pot_winner -- a double prefix over the winner's span
// partials, a bisection for the span, a walk inside it; no span reaches it: row N - 1; the walk does not (rounding between the two orders): the span's last row.
__global__ __launch_bounds__(kPickBlk) void kpp_pick_kernel(const float *__restrict__ mins, const double *__restrict__ part, int N, int S, int span, int T,
                                                             const int32_t *__restrict__ cand_ids, int id0, const double *__restrict__ u, int T_next,
                                                             int32_t *__restrict__ next_ids, int32_t *__restrict__ sel_out, int32_t *__restrict__ index_out,
                                                             int32_t *__restrict__ trace_ids, double *__restrict__ trace_pot, float *__restrict__ closest_out) {
    __shared__ double s_pot[kPpMaxT], s_wtot[kPpMaxT], s_inc[kPpMaxSpans];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (wv < T) {
        double v = 0.0;
        for (int s = lane; s < S; s += 64) v += part[(size_t)wv * S + s];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
        if (lane == 0) s_pot[wv] = v;
    }
    __syncthreads();
    int win = 0;
    double best = s_pot[0];
    for (int t = 1; t < T; ++t) {
        const double p = s_pot[t];
        if (p < best) { best = p; win = t; }
    }
    if (tid < T) {
        const int id = kpp_clamp(cand_ids ? cand_ids[tid] : id0, N);
        if (trace_ids) trace_ids[tid] = id;
        if (trace_pot) trace_pot[tid] = s_pot[tid];
        if (tid == win) { sel_out[0] = win; index_out[0] = id; }
    }
    const float *m = mins + (size_t)win * N;
    if (closest_out)
        for (int n = tid; n < N; n += kPickBlk) closest_out[n] = m[n];
    if (T_next <= 0) return;
    const double inc = kpp_wave_scan(tid < S ? part[(size_t)win * S + tid] : 0.0, lane);
    if (lane == 63) s_wtot[wv] = inc;
    __syncthreads();
    double before = 0.0;
    for (int w = 0; w < wv; ++w) before += s_wtot[w];
    s_inc[tid] = before + inc;
    __syncthreads();
    if (wv >= T_next) return;
    const double r = u[wv] * best;
    int lo = 0, hi = S;                                    // the first span whose inclusive prefix is >= r; S if none is (or r is a NaN)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (s_inc[mid] >= r) hi = mid; else lo = mid + 1;
    }
    int id = N - 1;
    if (lo < S) {
        double base = lo > 0 ? s_inc[lo - 1] : 0.0;
        const int begin = lo * span, end = min(N, begin + span);
        id = end - 1;
        bool found = false;
        for (int c0 = begin; c0 < end && !found; c0 += 64 * kPickRows) {
            float v[kPickRows];
#pragma unroll
            for (int q = 0; q < kPickRows; ++q) {
                const int row = c0 + q * 64 + lane;
                v[q] = row < end ? m[row] : 0.f;
            }
#pragma unroll
            for (int q = 0; q < kPickRows; ++q) {
                if (!found) {                              // the same in every lane
                    const double run = base + kpp_wave_scan((double)v[q], lane);
                    const unsigned long long hit = __ballot(c0 + q * 64 + lane < end && run >= r);
                    if (hit) { id = c0 + q * 64 + __ffsll((long long)hit) - 1; found = true; }
                    else base = __shfl(run, 63);
                }
            }
        }
    }
    if (lane == 0) next_ids[wv] = kpp_clamp(id, N);
}

bool km_rows(int64_t n) { return n <= 0x7fffffffll / 128; }

template <int D>
int kpp_dist_run(const float *X, int64_t N, const int32_t *cand_ids, int id0, int T, const float *closest_base, const int32_t *sel, int n_sel, float *mins,
                 double *part, hipStream_t st) {
    const int span = kpp_span(N), S = (int)((N + span - 1) / span);
#define KPP_DIST(TT)                                                                                                                         \
    hipLaunchKernelGGL((kpp_dist_kernel<D, TT>), dim3((unsigned)S), dim3(kBlk), 0, st, X, (int)N, span, cand_ids, id0, T, closest_base, sel, n_sel, mins, part, S)
    if (T <= 4) KPP_DIST(4);
    else if (T <= 8) KPP_DIST(8);
    else if (T <= 12) KPP_DIST(12);
    else KPP_DIST(16);
#undef KPP_DIST
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int kpp_dist(const float *X, int64_t N, int64_t d, const int32_t *cand_ids, int id0, int T, const float *closest_base, const int32_t *sel, int n_sel, float *mins,
             double *part, hipStream_t st) {
#define KPP_RUN(DD) return kpp_dist_run<DD>(X, N, cand_ids, id0, T, closest_base, sel, n_sel, mins, part, st)
    ARL_DISPATCH_WIDTH(d, KPP_RUN);
#undef KPP_RUN
}

int kpp_pick(const float *mins, const double *part, int64_t N, int T, const int32_t *cand_ids, int id0, const double *u, int T_next, int32_t *next_ids,
             int32_t *sel_out, int32_t *index_out, int32_t *trace_ids, double *trace_pot, float *closest_out, hipStream_t st) {
    const int span = kpp_span(N), S = (int)((N + span - 1) / span);
    hipLaunchKernelGGL(kpp_pick_kernel, dim3(1), dim3(kPickBlk), 0, st, mins, part, (int)N, S, span, T, cand_ids, id0, u, T_next, next_ids, sel_out, index_out,
                       trace_ids, trace_pot, closest_out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

// the whole-seeding workspace: part [T][S] double | ids [2][16] int32 | sel [4] int32 | mins [2][T][N] float
constexpr int64_t kPpIdsBytes = 2 * kPpMaxT * sizeof(int32_t), kPpSelBytes = 16;
int64_t kpp_part_bytes(int64_t N, int64_t T) { return ((int64_t)sizeof(double) * T * ((N + kpp_span(N) - 1) / kpp_span(N)) + 15) / 16 * 16; }

template <int D>
int km_assign_run(const float *X, int64_t N, const float *C, int64_t k, float *bias, int32_t *labels, float *score, hipStream_t st) {
    hipLaunchKernelGGL(km_bias_kernel, dim3((unsigned)((k + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, C, (int)k, D, bias);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL((km_assign_kernel<D>), dim3((unsigned)((N + 63) / 64)), dim3(kBlk), 0, st, X, (int)N, C, (const float *)bias, (int)k, labels, score);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // namespace

extern "C" {

int arl_kmeans_assign_f32(const float *X, int64_t N, const float *C, int64_t k, int64_t d, float *bias, int32_t *labels, float *score, arl_stream_t stream) {
    if (!X || !C || !bias || !labels || !score) return ARL_E_NULL;
    if (!arl_width_ok(d)) return ARL_E_DIM;
    if (N <= 0 || k <= 0) return ARL_E_ARG;
    if (N > 0x7fffffffll / 128 || k > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)X | (uintptr_t)C) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
#define KM_RUN(DD) return km_assign_run<DD>(X, N, C, k, bias, labels, score, st)
    ARL_DISPATCH_WIDTH(d, KM_RUN);
#undef KM_RUN
}

int64_t arl_kmeans_chunk_rows(void) { return kChunk; }

int64_t arl_kmeans_update_workspace_bytes(int64_t N, int64_t k, int64_t d) {
    if (N <= 0 || k <= 0 || !arl_width_ok(d)) return 0;
    return (int64_t)sizeof(float) * (N / kChunk + k) * d;          // sum_c ceil(count_c / kChunk) <= N / kChunk + k
}

int arl_kmeans_update_f32(const float *X, int64_t N, int64_t d, const int32_t *order, const int32_t *seg_ptr, const int32_t *chunk_ptr, int64_t k, const float *C_prev,
                          float *C_new, void *workspace, arl_stream_t stream) {
    if (!X || !order || !seg_ptr || !chunk_ptr || !C_prev || !C_new || !workspace) return ARL_E_NULL;
    if (!arl_width_ok(d)) return ARL_E_DIM;
    if (N <= 0 || k <= 0 || C_prev == C_new) return ARL_E_ARG;
    if (N > 0x7fffffffll / 128 || k > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)X | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(km_segsum_kernel, dim3((unsigned)(N / kChunk + k)), dim3(kBlk), 0, st, X, (int)N, (int)d, order, seg_ptr, chunk_ptr, (int)k, part);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_mean_kernel, dim3((unsigned)((k * d + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const float *)part, seg_ptr, chunk_ptr, (int)k, (int)d, C_prev, C_new);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_kmeans_sum_workspace_bytes(void) { return (int64_t)sizeof(double) * kSumParts; }

int arl_kmeans_sum_f64(const float *v, int64_t n, int32_t squared, double *out, void *workspace, arl_stream_t stream) {
    if (!v || !out || !workspace) return ARL_E_NULL;
    if (n <= 0) return ARL_E_ARG;
    if (((uintptr_t)out | (uintptr_t)workspace) & 7) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    long long parts = (n + 4095) / 4096;
    if (parts > kSumParts) parts = kSumParts;
    const long long span = (n + parts - 1) / parts;
    parts = (n + span - 1) / span;
    hipLaunchKernelGGL(km_sum_partial_kernel, dim3((unsigned)parts), dim3(kBlk), 0, st, v, (long long)n, span, (int)squared, (double *)workspace);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(km_sum_fold_kernel, dim3(1), dim3(kBlk), 0, st, (const double *)workspace, (int)parts, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_kmeanspp_spans(int64_t N) {
    if (N <= 0 || !km_rows(N)) return 0;
    return (N + kpp_span(N) - 1) / kpp_span(N);
}

int64_t arl_kmeanspp_span_rows(int64_t N) { return N <= 0 || !km_rows(N) ? 0 : kpp_span(N); }

int64_t arl_kmeanspp_workspace_bytes(int64_t N, int64_t n_trials) {
    if (N <= 0 || !km_rows(N) || n_trials < 1 || n_trials > kPpMaxT) return 0;
    return kpp_part_bytes(N, n_trials) + kPpIdsBytes + kPpSelBytes + (int64_t)sizeof(float) * 2 * n_trials * N;
}

int arl_kmeanspp_dist_f32(const float *X, int64_t N, int64_t d, const int32_t *cand_ids, int64_t n_cand, const float *closest, float *mins, double *part,
                          arl_stream_t stream) {
    if (!X || !cand_ids || !mins || !part) return ARL_E_NULL;
    if (!arl_width_ok(d)) return ARL_E_DIM;
    if (N <= 0 || n_cand < 1 || n_cand > kPpMaxT) return ARL_E_ARG;
    if (!km_rows(N)) return ARL_E_RANGE;
    if (((uintptr_t)X & 15) || ((uintptr_t)part & 7)) return ARL_E_ARG;
    return kpp_dist(X, N, d, cand_ids, 0, (int)n_cand, closest, nullptr, 1, mins, part, (hipStream_t)stream);
}

int arl_kmeanspp_pick_f64(const float *mins, const double *part, int64_t N, int64_t n_cand, const int32_t *cand_ids, const double *u, int64_t n_next,
                          int32_t *next_ids, int32_t *winner, double *cand_pot, float *closest_out, arl_stream_t stream) {
    if (!mins || !part || !cand_ids || !winner || !cand_pot || (n_next > 0 && (!u || !next_ids))) return ARL_E_NULL;
    if (N <= 0 || n_cand < 1 || n_cand > kPpMaxT || n_next < 0 || n_next > kPpMaxT) return ARL_E_ARG;
    if (!km_rows(N)) return ARL_E_RANGE;
    if (((uintptr_t)part | (uintptr_t)u | (uintptr_t)cand_pot) & 7) return ARL_E_ARG;
    return kpp_pick(mins, part, N, (int)n_cand, cand_ids, 0, u, (int)n_next, next_ids, winner, winner + 1, nullptr, cand_pot, closest_out, (hipStream_t)stream);
}

int arl_kmeanspp_f32(const float *X, int64_t N, int64_t d, int64_t k, int64_t n_trials, int64_t first, const double *u, int32_t *indices, float *closest,
                     int32_t *cand_ids, double *cand_pot, void *workspace, arl_stream_t stream) {
    if (!X || !indices || !closest || !workspace || (k > 1 && !u)) return ARL_E_NULL;
    if (!arl_width_ok(d)) return ARL_E_DIM;
    if (N <= 0 || k <= 0 || k > N || n_trials < 1 || n_trials > kPpMaxT || first < 0 || first >= N) return ARL_E_ARG;
    if (!km_rows(N) || !km_rows(k)) return ARL_E_RANGE;
    if ((((uintptr_t)X | (uintptr_t)workspace) & 15) || (((uintptr_t)u | (uintptr_t)cand_pot) & 7)) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int T = (int)n_trials;
    char *ws = (char *)workspace;
    double *part = (double *)ws;
    int32_t *ids = (int32_t *)(ws + kpp_part_bytes(N, T));
    int32_t *sel = ids + 2 * kPpMaxT;
    float *mins = (float *)(sel + 4);
    const size_t half = (size_t)T * N;
    // the first centre: closest = its distances (one candidate, no closest before it); the pick folds the potential and draws step 1's candidates
    int rc = kpp_dist(X, N, d, nullptr, (int)first, 1, nullptr, nullptr, 1, mins, part, st);
    if (rc != ARL_OK) return rc;
    rc = kpp_pick(mins, part, N, 1, nullptr, (int)first, u, k > 1 ? T : 0, ids, sel, indices, nullptr, nullptr, k > 1 ? nullptr : closest, st);
    for (int64_t c = 1; c < k && rc == ARL_OK; ++c) {
        const int32_t *cur = ids + ((c - 1) & 1) * kPpMaxT;
        float *out = mins + (c & 1) * half;
        const bool last = c == k - 1;
        rc = kpp_dist(X, N, d, cur, 0, T, mins + ((c - 1) & 1) * half, sel, T, out, part, st);
        if (rc != ARL_OK) return rc;
        rc = kpp_pick(out, part, N, T, cur, 0, last ? nullptr : u + c * T, last ? 0 : T, ids + (c & 1) * kPpMaxT, sel, indices + c,
                      cand_ids ? cand_ids + (c - 1) * T : nullptr, cand_pot ? cand_pot + (c - 1) * T : nullptr, last ? closest : nullptr, st);
    }
    return rc;
}

}  // extern "C"

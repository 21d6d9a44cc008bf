// arl_multinomial.hip -- the multinomial likelihood of the autoencoder recommenders (Mult-DAE / Mult-VAE, Liang et al., WWW'18): a softmax over EVERY
// item for each batch row, read at the row's positives, on gfx950 without any B x I tensor.
//
// With z = q E^T [B, I], lse_b = log sum_i exp z_bi, n_b = sum_{i in pos(b)} w_bi and p = softmax_i(z):
//     nll[b] = n_b lse_b - sum_{i in pos(b)} w_bi z_bi
//     dq[b]  = g_b ( n_b sum_i p_bi E_i - sum_{i in pos(b)} w_bi E_i )
//     dE[i]  = sum_b g_b ( n_b p_bi - w_bi [i in pos(b)] ) q_b
//
// Rules kept throughout:
//   * scores and the weighted row sums run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h);
//   * pass 1 (rows resident, items streamed in splits): the online row max and sum of exp, merged over the splits in ascending order;
//     pass 2 (one wave per row): lse, the sums over the row's CSR positives (their scores by the same instructions as the stream's), nll and the
//     row's dense coefficient a_b = g_b n_b;
//     pass 3 (rows resident): the dense part of dq, a_b sum_i p_bi E_i;   pass 4 (items resident, rows streamed in splits): the dense part of dE;
//     the two finishing kernels fold the splits in ascending order and subtract the sparse corrections, dq's over the row's positives and dE's over
//     the item's entries of the TRANSPOSED positives, each in list order;
//   * no atomics: every partial has one writer, so the outputs are bit-identical from run to run; sums over a stage's 64 streamed rows in fp32, over
//     the stages and the sparse lists in double;
//   * every workspace and output word is written before it is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
using strm::f32x4v;

enum { MN_STATS = 0, MN_DQ = 1, MN_DE = 2 };

// Xr [nR][D] resident, Xt [nT][D] streamed, split blockIdx.y takes the streamed rows
// [y split_len, (y + 1) split_len), split_len a multiple of 64.  In MN_STATS and MN_DQ the resident rows are the batch rows (q) and the streamed rows
// the items (E); in MN_DE the items are resident and the batch rows streamed.  stat [B][2] = (row max, 1 / row sum), coef [B] = g_b n_b.
//   MN_STATS: part_ms [split][nR][2] = the split's (max, sum of exp(z - max))
//   MN_DQ   : out [split][nR][D] = sum over the split's items of coef_b p_bi E[i]
//   MN_DE   : out [split][nR][D] = sum over the split's batch rows of coef_b p_bi q[b]
template <int D, int MODE>
__global__ __launch_bounds__(kBlk) void mn_stream_kernel(const float *__restrict__ Xr, int nR, const float *__restrict__ Xt, int nT, int split_len,
                                                          const float *__restrict__ stat, const float *__restrict__ coef, float *__restrict__ out,
                                                          float *__restrict__ part_ms) {
#pragma clang fp contract(off)
    constexpr int NT = D / 16;
    constexpr bool GRAD = MODE != MN_STATS;
    __shared__ float tile[2][strm::kStageFloats<D>];
    __shared__ float rsv[2][MODE == MN_DE ? 64 * 3 : 1];               // MN_DE: the streamed batch rows' (max, 1 / sum, coef)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(nT, t_begin + split_len);
    float br[D / 4];
    strm::load_resident<D>(Xr, r0 + c, nR, g, br);
    // the lane's batch row when the batch rows are resident
    const int brow_id = min(r0 + c, nR - 1);
    float rm = 0.f, rinv = 0.f, rco = 0.f;
    if (MODE == MN_DQ) { rm = stat[2 * (size_t)brow_id]; rinv = stat[2 * (size_t)brow_id + 1]; rco = coef[brow_id]; }
    f32x4v o[GRAD ? NT : 1];
    double o2[GRAD ? NT : 1][4];
#pragma unroll
    for (int n = 0; n < (GRAD ? NT : 1); ++n) {
        o[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o2[n][reg] = 0.0;
    }
    float sm = -INFINITY, ss = 0.f;                                      // MN_STATS
    const int nst = t_end > t_begin ? (t_end - t_begin + 63) / 64 : 0;
    // beside a stage's rows: MN_DE's statistics and coefficient of the streamed batch rows
    strm::stage<D> stg(tid);
    float pre_v[3] = {0.f, 0.f, 0.f};
#define MN_FETCH(ST)                                                                                                               \
    do {                                                                                                                           \
        stg.fetch(Xt, t_begin + (ST) * 64, nT);                                                                                    \
        if (MODE == MN_DE && tid < 64) {                                                                                           \
            const int t = min(t_begin + (ST) * 64 + tid, nT - 1);                                                                  \
            pre_v[0] = stat[2 * (size_t)t]; pre_v[1] = stat[2 * (size_t)t + 1]; pre_v[2] = coef[t];                                \
        }                                                                                                                          \
    } while (0)
#define MN_STASH(BUF)                                                                                                              \
    do {                                                                                                                           \
        stg.stash(tile[BUF]);                                                                                                      \
        if (MODE == MN_DE && tid < 64) {                                                                                           \
            _Pragma("unroll") for (int k = 0; k < 3; ++k) rsv[BUF][tid * 3 + k] = pre_v[k];                                        \
        }                                                                                                                          \
    } while (0)
    if (nst > 0) { MN_FETCH(0); MN_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) MN_FETCH(st + 1);
        const float *T = tile[buf];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f32x4v sc = strm::scores<D>(strm::a_row<D>(T, sub, c, g), br);
            const int tb = t_begin + st * 64 + sub * 16 + 4 * g;        // streamed row of register 0
            if (MODE == MN_STATS) {
                if (tb < t_end) {
                    float mx = sc[0];
#pragma unroll
                    for (int j = 1; j < 4; ++j) if (tb + j < t_end) mx = fmaxf(mx, sc[j]);
                    const float M = fmaxf(sm, mx);
                    float a = ss * expf(sm - M);
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (tb + j < t_end) a += expf(sc[j] - M);
                    ss = a; sm = M;
                }
                continue;
            }
            float pj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool live = tb + j < t_end;
                float m_ = rm, inv_ = rinv, co_ = rco;
                if (MODE == MN_DE) {
                    const float *v = rsv[buf] + (sub * 16 + 4 * g + j) * 3;
                    m_ = v[0]; inv_ = v[1]; co_ = v[2];
                }
                const float p = expf(sc[j] - m_) * inv_;
                pj[j] = live ? co_ * p : 0.f;
            }
            // strm::accumulate, written out: through the helper the items-resident form at d = 32 takes four more VGPRs and loses a wave of occupancy
            if constexpr (GRAD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float *brow = T + (sub * 16 + 4 * g + j) * strm::kLD<D> + c;
#pragma unroll
                    for (int n = 0; n < NT; ++n) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pj[j], brow[16 * n], o[n], 0, 0, 0);
                }
            }
        }
        if constexpr (GRAD) strm::flush_stage<D>(o, o2);
        if (st + 1 < nst) MN_STASH(buf ^ 1);
        __syncthreads();
    }
#undef MN_FETCH
#undef MN_STASH
    const size_t prow = (size_t)blockIdx.y * nR + (r0 + c);
    if (MODE == MN_STATS) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(sm, off), s2 = __shfl_xor(ss, off);
            strm::merge_lse(sm, ss, m2, s2);
        }
        if (g == 0 && r0 + c < nR) { part_ms[2 * prow] = sm; part_ms[2 * prow + 1] = ss; }
    }
    if constexpr (GRAD) strm::store_partial<D>(out, blockIdx.y, nR, r0, g, c, o2);
}

// One wave per batch row: the splits' (max, sum) states merged in ascending order, lse = max + log sum, then the row's positives 16 at a time: their
// scores z = <E_i, q_b> by the stream's own instruction sequence (the positives' rows of E as the A operand, q_b in every column of B), so a
// positive's z has the bits the dense passes saw -- at I = 1, nll = n z - w z is an exact 0 -- and n = sum w, sum w z in double, the entries in list
// order per lane group, the four groups folded by a fixed butterfly.  Writes stat [B][2] = (max, 1 / sum), lse, nll and coef [B] = g_b n_b (0 without g
// or without positives).
template <int D>
__global__ __launch_bounds__(kBlk) void mn_rows_kernel(const float *__restrict__ part_ms, int B, int ns, const float *__restrict__ q, const float *__restrict__ E,
                                                        const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                                        const float *__restrict__ gup, float *__restrict__ stat, float *__restrict__ lse, float *__restrict__ nll,
                                                        float *__restrict__ coef) {
#pragma clang fp contract(off)
    constexpr int Q = D / 4;
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4, b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= B) return;                                                  // wave-uniform
    float m = part_ms[2 * (size_t)b], s = part_ms[2 * (size_t)b + 1];
    for (int k = 1; k < ns; ++k) strm::merge_lse(m, s, part_ms[2 * ((size_t)k * B + b)], part_ms[2 * ((size_t)k * B + b) + 1]);
    const float l = m + logf(s);
    const int lo = rowptr[b], hi = rowptr[b + 1];
    float br[Q];
    strm::load_resident<D>(q, b, B, g, br);
    double n = 0.0, swz = 0.0;
    for (int e0 = lo; e0 < hi; e0 += 16) {                               // wave-uniform trip count
        const f32x4v sc = strm::scores<D>(E + (size_t)col[min(e0 + c, hi - 1)] * D + Q * g, br);
        if (c == 0) {                                                    // every column holds the same 16 scores: register j of group g is entry e0 + 4 g + j
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = e0 + 4 * g + j;
                if (e < hi) {
                    const double w = val ? (double)val[e] : 1.0;
                    n += w;
                    swz += w * (double)sc[j];
                }
            }
        }
    }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) { n += __shfl_xor(n, off); swz += __shfl_xor(swz, off); }
    if (lane == 0) {
        stat[2 * (size_t)b] = m; stat[2 * (size_t)b + 1] = 1.0f / s;
        lse[b] = l;
        nll[b] = hi > lo ? (float)(n * (double)l - swz) : 0.f;
        coef[b] = (gup && hi > lo) ? gup[b] * (float)n : 0.f;
    }
}

// dq[b][k] = (the splits' dense parts, ascending) - sum_{e in row b} (g_b w_e) E[col_e][k], the list in its own order, in double; the product g_b w_e is
// rounded to fp32 first, as the dense part's coefficient is, so that at I = 1 the two parts cancel exactly
template <int D>
__global__ __launch_bounds__(kBlk) void mn_finish_dq_kernel(const float *__restrict__ part, int B, int ns, const float *__restrict__ E, const int32_t *__restrict__ rowptr,
                                                             const int32_t *__restrict__ col, const float *__restrict__ val, const float *__restrict__ gup,
                                                             float *__restrict__ dq) {
#pragma clang fp contract(off)
    const size_t n = (size_t)B * D, e = (size_t)blockIdx.x * kBlk + threadIdx.x;
    if (e >= n) return;
    const int b = (int)(e / D), k = (int)(e % D);
    float v = part[e];
    for (int s = 1; s < ns; ++s) v += part[(size_t)s * n + e];
    double c = 0.0;
    const int lo = rowptr[b], hi = rowptr[b + 1];
    const float gb = gup[b];
    for (int t = lo; t < hi; ++t) {
        const float gw = val ? gb * val[t] : gb;
        c += (double)gw * (double)E[(size_t)col[t] * D + k];
    }
    dq[e] = hi > lo ? v - (float)c : 0.f;
}

// dE[i][k] = (the splits' dense parts, ascending) - sum_{t in item i's transposed entries} (g_b w_t) q[b][k], b = tcol[t], in list order, in double
template <int D>
__global__ __launch_bounds__(kBlk) void mn_finish_dE_kernel(const float *__restrict__ part, int I, int ns, const float *__restrict__ q, const int32_t *__restrict__ trowptr,
                                                             const int32_t *__restrict__ tcol, const int32_t *__restrict__ tperm, const float *__restrict__ val,
                                                             const float *__restrict__ gup, float *__restrict__ dE) {
#pragma clang fp contract(off)
    const size_t n = (size_t)I * D, e = (size_t)blockIdx.x * kBlk + threadIdx.x;
    if (e >= n) return;
    const int i = (int)(e / D), k = (int)(e % D);
    float v = part[e];
    for (int s = 1; s < ns; ++s) v += part[(size_t)s * n + e];
    double c = 0.0;
    const int lo = trowptr[i], hi = trowptr[i + 1];
    for (int t = lo; t < hi; ++t) {
        const int b = tcol[t];
        const float gw = val ? gup[b] * val[tperm[t]] : gup[b];
        c += (double)gw * (double)q[(size_t)b * D + k];
    }
    dE[e] = v - (float)c;
}

struct mn_layout { size_t part_ms, stat, coef, part_dq, part_dE, total; };
mn_layout mn_plan(int64_t B, int64_t I, int64_t d, bool grad) {
    const strm::split sq = strm::stage_splits(B, I), sb = strm::stage_splits(I, B);
    mn_layout L;
    size_t off = 0;
    L.part_ms = off; off += up16(sizeof(float) * 2 * (size_t)sq.ns * (size_t)B);
    L.stat = off; off += up16(sizeof(float) * 2 * (size_t)B);
    L.coef = off; off += up16(sizeof(float) * (size_t)B);
    L.part_dq = off; if (grad) off += up16(sizeof(float) * (size_t)sq.ns * (size_t)B * (size_t)d);
    L.part_dE = off; if (grad) off += up16(sizeof(float) * (size_t)sb.ns * (size_t)I * (size_t)d);
    L.total = off;
    return L;
}

template <int D>
int mn_run(const float *q, int64_t B, const float *E, int64_t I, const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *trowptr,
           const int32_t *tcol, const int32_t *tperm, const float *g, float *nll, float *lse, float *dq, float *dE, char *ws, hipStream_t st) {
    const bool grad = dq || dE;
    const mn_layout L = mn_plan(B, I, D, grad);
    const strm::split sq = strm::stage_splits(B, I), sb = strm::stage_splits(I, B);
    const dim3 blk(kBlk);
    float *stat = (float *)(ws + L.stat), *coef = (float *)(ws + L.coef);
    hipLaunchKernelGGL((mn_stream_kernel<D, MN_STATS>), dim3((unsigned)((B + 63) / 64), (unsigned)sq.ns), blk, 0, st, q, (int)B, E, (int)I, sq.len, (const float *)nullptr,
                       (const float *)nullptr, (float *)nullptr, (float *)(ws + L.part_ms));
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL((mn_rows_kernel<D>), dim3((unsigned)((B + kWaves - 1) / kWaves)), blk, 0, st, (const float *)(ws + L.part_ms), (int)B, sq.ns, q, E, rowptr, col, val,
                       grad ? g : (const float *)nullptr, stat, lse, nll, coef);
    ARL_LAUNCH_CHECK();
    if (dq) {
        float *part = (float *)(ws + L.part_dq);
        hipLaunchKernelGGL((mn_stream_kernel<D, MN_DQ>), dim3((unsigned)((B + 63) / 64), (unsigned)sq.ns), blk, 0, st, q, (int)B, E, (int)I, sq.len, (const float *)stat,
                           (const float *)coef, part, (float *)nullptr);
        ARL_LAUNCH_CHECK();
        const size_t n = (size_t)B * D;
        hipLaunchKernelGGL((mn_finish_dq_kernel<D>), dim3((unsigned)((n + kBlk - 1) / kBlk)), blk, 0, st, (const float *)part, (int)B, sq.ns, E, rowptr, col, val, g, dq);
        ARL_LAUNCH_CHECK();
    }
    if (dE) {
        float *part = (float *)(ws + L.part_dE);
        hipLaunchKernelGGL((mn_stream_kernel<D, MN_DE>), dim3((unsigned)((I + 63) / 64), (unsigned)sb.ns), blk, 0, st, E, (int)I, q, (int)B, sb.len, (const float *)stat,
                           (const float *)coef, part, (float *)nullptr);
        ARL_LAUNCH_CHECK();
        const size_t n = (size_t)I * D;
        hipLaunchKernelGGL((mn_finish_dE_kernel<D>), dim3((unsigned)((n + kBlk - 1) / kBlk)), blk, 0, st, (const float *)part, (int)I, sb.ns, q, trowptr, tcol, tperm, val, g, dE);
        ARL_LAUNCH_CHECK();
    }
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_multinomial_softmax_workspace_bytes(int64_t B, int64_t I, int64_t d, int32_t want_grad) {
    if (!strm::shape_ok(B, I, d)) return 0;
    return (int64_t)mn_plan(B, I, d, want_grad != 0).total;
}

int arl_multinomial_softmax_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const int32_t *rowptr, const int32_t *col, const float *val, int64_t nnz,
                                const int32_t *trowptr, const int32_t *tcol, const int32_t *tperm, const float *g, float *nll, float *lse, float *dq, float *dE,
                                void *workspace, arl_stream_t stream) {
    if (!q || !E || !rowptr || !col || !nll || !lse || !workspace) return ARL_E_NULL;
    if ((dq || dE) && !g) return ARL_E_NULL;
    if (dE && (!trowptr || !tcol || (val && !tperm))) return ARL_E_NULL;
    if (d != 16 && d != 32 && d != 64 && d != 128) return ARL_E_DIM;
    if (B <= 0 || I <= 0 || nnz < 0) return ARL_E_ARG;
    if (B > 0x7fffffffll / 128 || I > 0x7fffffffll / 128 || nnz > 0x7fffffffll) return ARL_E_RANGE;
    if (((uintptr_t)q | (uintptr_t)E | (uintptr_t)dq | (uintptr_t)dE | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define MN_RUN(DD) return mn_run<DD>(q, B, E, I, rowptr, col, val, trowptr, tcol, tperm, g, nll, lse, dq, dE, ws, st)
    ARL_DISPATCH_WIDTH(d, MN_RUN);
#undef MN_RUN
}

}  // extern "C"

// arl_policyhead.hip -- PoisonRec's policy head (reference attack/Black/PoisonRec.py:363-371, 398-401): a Bernoulli distribution over every item whose
// logits are the softmax probabilities of z = q E^T [B, I], on gfx950 without any B x I tensor.
//
// With p = softmax_i(z), sp = softplus(p), sg = sigmoid(p) and packed action bits a (bit i % 32 of word i / 32 of a row is item i):
//     logp[b] = sum_i (a p - sp),     ent[b] = sum_i (sp - p sg),
//     c_i = gl (a_i - sg_i) - ge p_i sg_i (1 - sg_i),     t_b = sum_j p_j c_j,     dz_i = p_i (c_i - t_b),     dq = dz E,     dE = dz^T q.
//
// Rules kept throughout:
//   * scores and the weighted row sums run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h);
//   * pass 1 (rows resident, items streamed in splits): the online row max and sum of exp, merged over the splits in ascending order;
//     pass 2: the row sums logp, ent, t (or, sampling: the action bits, logp and the count);   pass 3: dq;   pass 4 (items resident, rows streamed in
//     splits): dE.  Item splits are whole 64-item stages, so one lane writes each action word; B = 1 is spread over the chip by the splits, and
//     the splits of passes 1 and 2 depend on I alone, so a row's statistics and sampled bits are the same in a B-row call and a call of its own;
//   * no atomics: every partial has one writer and is folded in ascending split order, so the outputs are bit-identical from run to run; sums over
//     a stage's 64 streamed rows in fp32, over the stages and the splits in double;
//   * every workspace and output word is written before it is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
using strm::f32x4v;

// arl_profilegen.hip's row key with round 0: the draw at (row, i) is a function of (seed, call, row, i) only
__device__ __forceinline__ uint64_t ph_rowkey(uint64_t key, int row) { return arl_splitmix64(key ^ (uint64_t)(uint32_t)row); }
// u = n 2^-24 for the 24-bit draw n: exact in fp32, in [0, 1)
__device__ __forceinline__ float ph_uniform(uint64_t rowkey, int i) {
    return (float)(uint32_t)(arl_splitmix64(rowkey ^ (uint64_t)(uint32_t)i) >> 40) * (1.0f / 16777216.0f);
}

// p = exp(z - m) / s, sg = sigmoid(p), sp = softplus(p) = p + log1p(exp(-p)) for p in [0, 1].  Contraction is off so that every pass gets the same bits.
__device__ __forceinline__ void ph_terms(float z, float m, float inv, float &p, float &sg, float &sp) {
#pragma clang fp contract(off)
    p = expf(z - m) * inv;
    const float en = expf(-p);
    sg = 1.0f / (1.0f + en);
    sp = p + log1pf(en);
}

enum { PH_STATS = 0, PH_SUMS = 1, PH_SAMPLE = 2, PH_DQ = 3, PH_DE = 4 };
enum { PH_U_TENSOR = 0, PH_U_HASH = 1, PH_U_MODE = 2 };

// Xr [nR][D] resident, Xt [nT][D] streamed, split blockIdx.y takes the streamed rows
// [y split_len, (y + 1) split_len).  In every mode but PH_DE the resident rows are the batch rows (q) and the streamed rows the items (E), and split_len
// is a multiple of 64; in PH_DE the items are resident and the batch rows streamed.  stat [B][2] = (row max, 1 / row sum).
//   PH_STATS : part_ms [split][nR][2] = the split's (max, sum of exp(z - max))
//   PH_SUMS  : part_sum [split][nR][3] = the split's (sum a p - sp, sum sp - p sg, sum p c)
//   PH_SAMPLE: act_out words of the split's items, part_sum [split][nR][3] = (sum a p - sp, number of set bits, 0)
//   PH_DQ    : out [split][nR][D] = sum over the split's items of dz E[i]
//   PH_DE    : out [split][nR][D] = sum over the split's batch rows of dz q[b]
template <int D, int MODE>
__global__ __launch_bounds__(kBlk) void ph_stream_kernel(const float *__restrict__ Xr, int nR, const float *__restrict__ Xt, int nT, int split_len,
                                                          const float *__restrict__ stat, const float *__restrict__ gl, const float *__restrict__ ge,
                                                          const float *__restrict__ tt, const uint32_t *__restrict__ act, uint32_t *__restrict__ act_out, int W,
                                                          const float *__restrict__ u, uint64_t key, int row0, int usrc, float *__restrict__ out,
                                                          float *__restrict__ part_ms, double *__restrict__ part_sum) {
#pragma clang fp contract(off)
    constexpr int NT = D / 16;
    constexpr bool GRAD = MODE == PH_DQ || MODE == PH_DE, ROWS = MODE != PH_DE, BITS = MODE == PH_SUMS || MODE == PH_DQ;
    __shared__ float tile[2][strm::kStageFloats<D>];
    __shared__ float rsv[2][MODE == PH_DE ? 64 * 5 : 1];               // PH_DE: the streamed batch rows' (max, 1 / sum, gl, ge, t)
    __shared__ uint32_t rsw[2][MODE == PH_DE ? 64 * 2 : 1];            // PH_DE: their two action words over this workgroup's 64 items
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(nT, t_begin + split_len);
    float br[D / 4];
    strm::load_resident<D>(Xr, r0 + c, nR, g, br);
    // the lane's batch row when the batch rows are resident
    const int brow_id = min(r0 + c, nR - 1);
    float rm = 0.f, rinv = 0.f, rgl = 0.f, rge = 0.f, rt = 0.f;
    if (ROWS && MODE != PH_STATS) {
        rm = stat[2 * (size_t)brow_id]; rinv = stat[2 * (size_t)brow_id + 1];
        if (MODE != PH_SAMPLE) {
            rgl = gl ? gl[brow_id] : 0.f; rge = ge ? ge[brow_id] : 0.f;
            if (MODE == PH_DQ) rt = tt[brow_id];
        }
    }
    const uint64_t rowkey = (MODE == PH_SAMPLE && usrc == PH_U_HASH) ? ph_rowkey(key, row0 + brow_id) : 0ull;
    f32x4v o[GRAD ? NT : 1];
    double o2[GRAD ? NT : 1][4];
#pragma unroll
    for (int n = 0; n < (GRAD ? NT : 1); ++n) {
        o[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o2[n][reg] = 0.0;
    }
    float sm = -INFINITY, ss = 0.f;                                      // PH_STATS
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;                           // PH_SUMS / PH_SAMPLE
    int cnt = 0;
    const int nst = t_end > t_begin ? (t_end - t_begin + 63) / 64 : 0;
    // beside a stage's rows: PH_DE's statistics and action words of the streamed batch rows, BITS' action words of the lane's own row
    strm::stage<D> stg(tid);
    float pre_v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    uint32_t pre_w[2] = {0u, 0u};
    uint32_t aw_next[2] = {0u, 0u}, aw[2] = {0u, 0u};                    // BITS: the lane's batch row's two action words of a stage
    const int W0 = 2 * blockIdx.x;                                       // PH_DE: the first action word of this workgroup's items
#define PH_FETCH(ST)                                                                                                               \
    do {                                                                                                                           \
        stg.fetch(Xt, t_begin + (ST) * 64, nT);                                                                                    \
        if (MODE == PH_DE && tid < 64) {                                                                                           \
            const int t = min(t_begin + (ST) * 64 + tid, nT - 1);                                                                  \
            pre_v[0] = stat[2 * (size_t)t]; pre_v[1] = stat[2 * (size_t)t + 1]; pre_v[2] = gl[t]; pre_v[3] = ge[t]; pre_v[4] = tt[t]; \
            pre_w[0] = W0 < W ? act[(size_t)t * W + W0] : 0u;                                                                      \
            pre_w[1] = W0 + 1 < W ? act[(size_t)t * W + W0 + 1] : 0u;                                                              \
        }                                                                                                                          \
        if (BITS) {                                                                                                                \
            const int w0 = 2 * (t_begin / 64 + (ST));                                                                              \
            aw_next[0] = w0 < W ? act[(size_t)brow_id * W + w0] : 0u;                                                              \
            aw_next[1] = w0 + 1 < W ? act[(size_t)brow_id * W + w0 + 1] : 0u;                                                      \
        }                                                                                                                          \
    } while (0)
#define PH_STASH(BUF)                                                                                                              \
    do {                                                                                                                           \
        stg.stash(tile[BUF]);                                                                                                      \
        if (MODE == PH_DE && tid < 64) {                                                                                           \
            _Pragma("unroll") for (int k = 0; k < 5; ++k) rsv[BUF][tid * 5 + k] = pre_v[k];                                        \
            rsw[BUF][tid * 2] = pre_w[0]; rsw[BUF][tid * 2 + 1] = pre_w[1];                                                        \
        }                                                                                                                          \
    } while (0)
    if (nst > 0) { PH_FETCH(0); PH_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        aw[0] = aw_next[0]; aw[1] = aw_next[1];
        if (st + 1 < nst) PH_FETCH(st + 1);
        const float *T = tile[buf];
        float st0 = 0.f, st1 = 0.f, st2 = 0.f;
        uint32_t wbits[2] = {0u, 0u};
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f32x4v sc = strm::scores<D>(strm::a_row<D>(T, sub, c, g), br);
            const int tb = t_begin + st * 64 + sub * 16 + 4 * g;        // streamed row of register 0
            if (MODE == PH_STATS) {
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
            float pj[4], f0[4], f1[4], f2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool live = tb + j < t_end;
                const int sr = sub * 16 + 4 * g + j;                     // the streamed row's place in the stage
                float m_ = rm, inv_ = rinv, gl_ = rgl, ge_ = rge, t_ = rt;
                bool a = false;
                if (MODE == PH_DE) {
                    const float *v = rsv[buf] + sr * 5;
                    m_ = v[0]; inv_ = v[1]; gl_ = v[2]; ge_ = v[3]; t_ = v[4];
                    a = (rsw[buf][sr * 2 + (wv >> 1)] >> ((wv & 1) * 16 + c)) & 1u;
                } else if (BITS) {
                    a = (aw[sub >> 1] >> ((sub & 1) * 16 + 4 * g + j)) & 1u;
                }
                float p, sg, sp;
                ph_terms(sc[j], m_, inv_, p, sg, sp);
                if (MODE == PH_SAMPLE) {
                    if (usrc == PH_U_MODE) a = p > 0.f;
                    else {
                        float uu = 2.f;
                        if (usrc == PH_U_HASH) uu = ph_uniform(rowkey, tb + j);
                        else if (live) uu = u[(size_t)brow_id * nT + tb + j];
                        a = uu < sg;
                    }
                    a = a && live;
                    if (a) { wbits[sub >> 1] |= 1u << ((sub & 1) * 16 + 4 * g + j); ++cnt; }
                    f0[j] = live ? (a ? p : 0.f) - sp : 0.f;
                } else {
                    const float cc = gl_ * ((a ? 1.f : 0.f) - sg) - ge_ * (p * sg * (1.f - sg));
                    if (MODE == PH_SUMS) {
                        f0[j] = live ? (a ? p : 0.f) - sp : 0.f;
                        f1[j] = live ? sp - p * sg : 0.f;
                        f2[j] = live ? p * cc : 0.f;
                    } else {
                        pj[j] = live ? p * (cc - t_) : 0.f;
                    }
                }
            }
            if (MODE == PH_SUMS || MODE == PH_SAMPLE) st0 += (f0[0] + f0[1]) + (f0[2] + f0[3]);
            if (MODE == PH_SUMS) { st1 += (f1[0] + f1[1]) + (f1[2] + f1[3]); st2 += (f2[0] + f2[1]) + (f2[2] + f2[3]); }
            if constexpr (GRAD) strm::accumulate<D>(T, sub, c, g, pj, o);
        }
        if (MODE == PH_SUMS || MODE == PH_SAMPLE) acc0 += (double)st0;   // 16 scores in fp32, the stages in double
        if (MODE == PH_SUMS) { acc1 += (double)st1; acc2 += (double)st2; }
        if (MODE == PH_SAMPLE) {
            // the four lane groups of a batch row hold disjoint bits of the stage's two words; one lane writes them
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                uint32_t v = wbits[k];
                v |= (uint32_t)__shfl_xor((int)v, 16);
                v |= (uint32_t)__shfl_xor((int)v, 32);
                const int w = 2 * (t_begin / 64 + st) + k;
                if (g == 0 && r0 + c < nR && w < W) act_out[(size_t)(r0 + c) * W + w] = v;
            }
        }
        if constexpr (GRAD) strm::flush_stage<D>(o, o2);
        if (st + 1 < nst) PH_STASH(buf ^ 1);
        __syncthreads();
    }
#undef PH_FETCH
#undef PH_STASH
    const size_t prow = (size_t)blockIdx.y * nR + (r0 + c);
    if (MODE == PH_STATS) {
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(sm, off), s2 = __shfl_xor(ss, off);
            strm::merge_lse(sm, ss, m2, s2);
        }
        if (g == 0 && r0 + c < nR) { part_ms[2 * prow] = sm; part_ms[2 * prow + 1] = ss; }
    }
    if (MODE == PH_SUMS || MODE == PH_SAMPLE) {
        if (MODE == PH_SAMPLE) acc1 = (double)cnt;
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            acc0 += __shfl_xor(acc0, off); acc1 += __shfl_xor(acc1, off); acc2 += __shfl_xor(acc2, off);
        }
        if (g == 0 && r0 + c < nR) { part_sum[3 * prow] = acc0; part_sum[3 * prow + 1] = acc1; part_sum[3 * prow + 2] = acc2; }
    }
    if constexpr (GRAD) strm::store_partial<D>(out, blockIdx.y, nR, r0, g, c, o2);
}

// stat [B][2] = (max, 1 / sum) from the splits' states, ascending
__global__ __launch_bounds__(kBlk) void ph_merge_stats_kernel(const float *__restrict__ part_ms, int B, int ns, float *__restrict__ stat) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * kBlk + threadIdx.x;
    if (b >= B) return;
    float m = part_ms[2 * (size_t)b], s = part_ms[2 * (size_t)b + 1];
    for (int k = 1; k < ns; ++k) strm::merge_lse(m, s, part_ms[2 * ((size_t)k * B + b)], part_ms[2 * ((size_t)k * B + b) + 1]);
    stat[2 * (size_t)b] = m;
    stat[2 * (size_t)b + 1] = 1.0f / s;
}

// the splits' row sums, ascending, in double.  o0 = slot 0; o1 (float) / oc (int32) = slot 1; o2 = slot 2; NULL skips
__global__ __launch_bounds__(kBlk) void ph_finish_sums_kernel(const double *__restrict__ part_sum, int B, int ns, float *__restrict__ o0, float *__restrict__ o1,
                                                               int32_t *__restrict__ oc, float *__restrict__ o2) {
    const int b = blockIdx.x * kBlk + threadIdx.x;
    if (b >= B) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int k = 0; k < ns; ++k) {
        const double *p = part_sum + 3 * ((size_t)k * B + b);
        a0 += p[0]; a1 += p[1]; a2 += p[2];
    }
    if (o0) o0[b] = (float)a0;
    if (o1) o1[b] = (float)a1;
    if (oc) oc[b] = (int32_t)a1;
    if (o2) o2[b] = (float)a2;
}

// out[e] = sum over the splits of part[k][e], ascending
__global__ __launch_bounds__(kBlk) void ph_fold_kernel(const float *__restrict__ part, size_t n, int ns, float *__restrict__ out) {
    const size_t e = (size_t)blockIdx.x * kBlk + threadIdx.x;
    if (e >= n) return;
    float v = part[e];
    for (int k = 1; k < ns; ++k) v += part[(size_t)k * n + e];
    out[e] = v;
}

__global__ __launch_bounds__(kBlk) void ph_uniforms_kernel(uint64_t key, int row0, int I, int ntiles, float *__restrict__ out) {
    const int b = blockIdx.x / ntiles, i = (blockIdx.x % ntiles) * kBlk + threadIdx.x;
    if (i >= I) return;
    out[(size_t)b * I + i] = ph_uniform(ph_rowkey(key, row0 + b), i);
}

// the dq and dE streams split by strm::stage_splits
using ph_split = strm::split;

// splits of the items for the row statistics, the row sums and the sampling pass: a function of I alone (at least 1 024 items each, whole stages), so
// a row's statistics, and with them its sampled bits, do not depend on how many rows the call has.  A one-row call is a chain of stages per
// workgroup: 1 024 items are 16 of them (2 048 measured 0.33 ms for the three launches at one row against the composed route's 0.23 ms)
ph_split ph_item_splits(int64_t I) {
    int64_t s = (I + 1023) / 1024;
    if (s > 256) s = 256;
    const int64_t len = ((I + s - 1) / s + 63) / 64 * 64;
    return ph_split{(int)((I + len - 1) / len), (int)len};
}

struct ph_layout { size_t part_ms, stat, part_sum, tt, part_dq, part_dE, total; };
ph_layout ph_plan(int64_t B, int64_t I, int64_t d, bool grad) {
    const ph_split si = ph_item_splits(I), sq = strm::stage_splits(B, I), sb = strm::stage_splits(I, B);
    ph_layout L;
    size_t off = 0;
    L.part_ms = off; off += up16(sizeof(float) * 2 * (size_t)si.ns * (size_t)B);
    L.stat = off; off += up16(sizeof(float) * 2 * (size_t)B);
    L.part_sum = off; off += up16(sizeof(double) * 3 * (size_t)si.ns * (size_t)B);
    L.tt = off; off += up16(sizeof(float) * (size_t)B);
    L.part_dq = off; if (grad && sq.ns > 1) off += up16(sizeof(float) * (size_t)sq.ns * (size_t)B * (size_t)d);
    L.part_dE = off; if (grad && sb.ns > 1) off += up16(sizeof(float) * (size_t)sb.ns * (size_t)I * (size_t)d);
    L.total = off;
    return L;
}

template <int D>
int ph_stats(const float *q, int64_t B, const float *E, int64_t I, char *ws, const ph_layout &L, const ph_split &si, hipStream_t st) {
    const dim3 blk(kBlk), grid((unsigned)((B + 63) / 64), (unsigned)si.ns), rows((unsigned)((B + kBlk - 1) / kBlk));
    hipLaunchKernelGGL((ph_stream_kernel<D, PH_STATS>), grid, blk, 0, st, q, (int)B, E, (int)I, si.len, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, 0, (const float *)nullptr, 0ull, 0, 0,
                       (float *)nullptr, (float *)(ws + L.part_ms), (double *)nullptr);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ph_merge_stats_kernel, rows, blk, 0, st, (const float *)(ws + L.part_ms), (int)B, si.ns, (float *)(ws + L.stat));
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

template <int D>
int ph_eval(const float *q, int64_t B, const float *E, int64_t I, const uint32_t *act, const float *gl, const float *ge, float *logp, float *ent, float *dq,
            float *dE, char *ws, hipStream_t st) {
    const bool grad = dq || dE;
    const ph_layout L = ph_plan(B, I, D, grad);
    const ph_split si = ph_item_splits(I), sq = strm::stage_splits(B, I), sb = strm::stage_splits(I, B);
    const int W = (int)((I + 31) / 32);
    const dim3 blk(kBlk), grid((unsigned)((B + 63) / 64), (unsigned)si.ns), rows((unsigned)((B + kBlk - 1) / kBlk));
    const float *stat = (const float *)(ws + L.stat);
    float *tt = (float *)(ws + L.tt);
    int rc = ph_stats<D>(q, B, E, I, ws, L, si, st);
    if (rc != ARL_OK) return rc;
    hipLaunchKernelGGL((ph_stream_kernel<D, PH_SUMS>), grid, blk, 0, st, q, (int)B, E, (int)I, si.len, stat, gl, ge, (const float *)nullptr, act, (uint32_t *)nullptr, W,
                       (const float *)nullptr, 0ull, 0, 0, (float *)nullptr, (float *)nullptr, (double *)(ws + L.part_sum));
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ph_finish_sums_kernel, rows, blk, 0, st, (const double *)(ws + L.part_sum), (int)B, si.ns, logp, ent, (int32_t *)nullptr, tt);
    ARL_LAUNCH_CHECK();
    if (dq) {
        float *dst = sq.ns > 1 ? (float *)(ws + L.part_dq) : dq;
        hipLaunchKernelGGL((ph_stream_kernel<D, PH_DQ>), dim3((unsigned)((B + 63) / 64), (unsigned)sq.ns), blk, 0, st, q, (int)B, E, (int)I, sq.len, stat, gl, ge, (const float *)tt, act, (uint32_t *)nullptr, W,
                           (const float *)nullptr, 0ull, 0, 0, dst, (float *)nullptr, (double *)nullptr);
        ARL_LAUNCH_CHECK();
        if (sq.ns > 1) {
            const size_t n = (size_t)B * D;
            hipLaunchKernelGGL(ph_fold_kernel, dim3((unsigned)((n + kBlk - 1) / kBlk)), blk, 0, st, (const float *)dst, n, sq.ns, dq);
            ARL_LAUNCH_CHECK();
        }
    }
    if (dE) {
        float *dst = sb.ns > 1 ? (float *)(ws + L.part_dE) : dE;
        hipLaunchKernelGGL((ph_stream_kernel<D, PH_DE>), dim3((unsigned)((I + 63) / 64), (unsigned)sb.ns), blk, 0, st, E, (int)I, q, (int)B, sb.len, stat, gl, ge,
                           (const float *)tt, act, (uint32_t *)nullptr, W, (const float *)nullptr, 0ull, 0, 0, dst, (float *)nullptr, (double *)nullptr);
        ARL_LAUNCH_CHECK();
        if (sb.ns > 1) {
            const size_t n = (size_t)I * D;
            hipLaunchKernelGGL(ph_fold_kernel, dim3((unsigned)((n + kBlk - 1) / kBlk)), blk, 0, st, (const float *)dst, n, sb.ns, dE);
            ARL_LAUNCH_CHECK();
        }
    }
    return ARL_OK;
}

template <int D>
int ph_sample(const float *q, int64_t B, const float *E, int64_t I, const float *u, uint64_t key, int64_t row0, int usrc, uint32_t *act, float *logp, int32_t *count,
              char *ws, hipStream_t st) {
    const ph_layout L = ph_plan(B, I, D, false);
    const ph_split si = ph_item_splits(I);
    const int W = (int)((I + 31) / 32);
    const dim3 blk(kBlk), grid((unsigned)((B + 63) / 64), (unsigned)si.ns), rows((unsigned)((B + kBlk - 1) / kBlk));
    int rc = ph_stats<D>(q, B, E, I, ws, L, si, st);
    if (rc != ARL_OK) return rc;
    hipLaunchKernelGGL((ph_stream_kernel<D, PH_SAMPLE>), grid, blk, 0, st, q, (int)B, E, (int)I, si.len, (const float *)(ws + L.stat), (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, (const uint32_t *)nullptr, act, W, u, key, (int)row0, usrc, (float *)nullptr, (float *)nullptr,
                       (double *)(ws + L.part_sum));
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(ph_finish_sums_kernel, rows, blk, 0, st, (const double *)(ws + L.part_sum), (int)B, si.ns, logp, (float *)nullptr, count, (float *)nullptr);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_bernoulli_softmax_workspace_bytes(int64_t B, int64_t I, int64_t d, int32_t want_grad) {
    if (!strm::shape_ok(B, I, d)) return 0;
    return (int64_t)ph_plan(B, I, d, want_grad != 0).total;
}

int arl_bernoulli_softmax_eval_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const int32_t *actions, const float *gl, const float *ge,
                                   float *logp, float *ent, float *dq, float *dE, void *workspace, arl_stream_t stream) {
    if (!q || !E || !actions || !logp || !ent || !workspace) return ARL_E_NULL;
    if ((dq || dE) && (!gl || !ge)) return ARL_E_NULL;
    if (d != 16 && d != 32 && d != 64 && d != 128) return ARL_E_DIM;
    if (B <= 0 || I <= 0) return ARL_E_ARG;
    if (B > 0x7fffffffll / 128 || I > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)q | (uintptr_t)E | (uintptr_t)dq | (uintptr_t)dE | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const uint32_t *act = (const uint32_t *)actions;
#define PH_RUN(DD) return ph_eval<DD>(q, B, E, I, act, gl, ge, logp, ent, dq, dE, ws, st)
    ARL_DISPATCH_WIDTH(d, PH_RUN);
#undef PH_RUN
}

int arl_bernoulli_softmax_sample_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const float *u, uint64_t seed, uint64_t call, int64_t row0,
                                     int32_t deterministic, int32_t *actions, float *logp, int32_t *count, void *workspace, arl_stream_t stream) {
    if (!q || !E || !actions || !logp || !count || !workspace) return ARL_E_NULL;
    if (d != 16 && d != 32 && d != 64 && d != 128) return ARL_E_DIM;
    if (B <= 0 || I <= 0 || row0 < 0) return ARL_E_ARG;
    if (B > 0x7fffffffll / 128 || I > 0x7fffffffll / 128 || row0 + B > 0x7fffffffll) return ARL_E_RANGE;
    if (((uintptr_t)q | (uintptr_t)E | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
    const int usrc = deterministic ? PH_U_MODE : (u ? PH_U_TENSOR : PH_U_HASH);
    const uint64_t key = arl_gan_hash_key(seed, call);
#define PH_RUN(DD) return ph_sample<DD>(q, B, E, I, u, key, row0, usrc, (uint32_t *)actions, logp, count, ws, st)
    ARL_DISPATCH_WIDTH(d, PH_RUN);
#undef PH_RUN
}

int arl_bernoulli_uniforms_f32(uint64_t seed, uint64_t call, int64_t row0, int64_t B, int64_t I, float *out, arl_stream_t stream) {
    if (!out) return ARL_E_NULL;
    if (B <= 0 || I <= 0 || row0 < 0) return ARL_E_ARG;
    const int64_t ntiles = (I + kBlk - 1) / kBlk;
    if (I > 0x7fffffffll - kBlk || row0 + B > 0x7fffffffll || B * ntiles > 0x7fffffffll) return ARL_E_RANGE;
    hipLaunchKernelGGL(ph_uniforms_kernel, dim3((unsigned)(B * ntiles)), dim3(kBlk), 0, (hipStream_t)stream, arl_gan_hash_key(seed, call), (int)row0, (int)I, (int)ntiles, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

// arl_allpairs.hip -- GSPAttack's L_per (reference attack/Black/GSPAttack.py:63-75): a binary cross-entropy over EVERY score of s = Pu Pi^T [R, I]
// against a sparse target matrix a, on gfx950 without the R x I score matrix.
//
// With p = sigmoid(s), q = sigmoid(-s) (the reference's 1 - sigmoid(s)), f0(s) = -log(q + eps), f1(s) = -log(p + eps):
//     bce(s, a) = a f1(s) + (1 - a) f0(s),     rowloss[r] = sum_i f0(s[r, i]) + sum_{(r, c) listed} a (f1 - f0)(s[r, c]),     loss = sum_r rw[r] rowloss[r],
//     f0' = p q / (q + eps),  f1' = -p q / (p + eps),     g[r, i] = f0' + a (f1' - f0'),
//     dPu[r] = upstream rw[r] sum_i g[r, i] Pi[i],     dPi[i] = upstream sum_r rw[r] g[r, i] Pu[r].
// So the loss is a dense stream over all R x I scores (f0 only) plus a correction over the listed positives.
//
// Rules kept throughout:
//   * scores and the weighted row sums of the dense stream run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h),
//     the streamed rows' row_weight beside each stage;
//   * pass 1: users resident, all items streamed: rowloss and the raw dPu, one writer per row;   pass 2: items resident, users streamed in splits:
//     raw dPi partials;   pass 3: two gather kernels over the positives, a wave per row (by user: finishes rowloss and dPu; by item: folds the splits
//     in ascending order and finishes dPi), lane groups in a fixed order;
//   * no atomics: bit-identical from run to run; the loss-only call runs the same arithmetic as the gradient call; scalar sums in double, and so
//     are the sums over the stream's 64-row stages (rowloss and the weighted row sums).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
using strm::f32x4v;

// p = sigmoid(s) and q = sigmoid(-s) from one exp of -|s|: neither is rounded from 1 - the other.  Contraction is off so that every kernel that
// calls these gets the same bits (the loss-only and the gradient instantiations, the by-user and the by-item gathers).
__device__ __forceinline__ void bap_sigmoids(float s, float &p, float &q) {
#pragma clang fp contract(off)
    const float e = expf(-fabsf(s));
    const float t = 1.0f / (1.0f + e);
    const float et = e * t;
    p = s >= 0.f ? t : et;
    q = s >= 0.f ? et : t;
}

// f0 = -log(q + eps) and its derivative w0 = p q / (q + eps)
__device__ __forceinline__ void bap_dense_terms(float s, float eps, float &f0, float &w0) {
#pragma clang fp contract(off)
    float p, q;
    bap_sigmoids(s, p, q);
    const float qe = q + eps;
    f0 = -logf(qe);
    w0 = (p * q) / qe;
}

// what a listed positive adds per unit of its weight: df = f1 - f0, dw = f1' - f0'
__device__ __forceinline__ void bap_positive_terms(float s, float eps, float &df, float &dw) {
#pragma clang fp contract(off)
    float p, q;
    bap_sigmoids(s, p, q);
    const float qe = q + eps, pe = p + eps, pq = p * q;
    df = logf(qe) - logf(pe);
    dw = -(pq / pe) - (pq / qe);
}

enum { BAP_ROWS_LOSS = 0, BAP_ROWS_GRAD = 1, BAP_COLS_GRAD = 2 };

// MODE BAP_ROWS_LOSS: rowloss[r] = sum over the streamed rows t of f0(<Xr[r], Xt[t]>)                                     (gridDim.y = 1)
// MODE BAP_ROWS_GRAD: the same, and out [nR][D] = sum_t f0'(s[r, t]) Xt[t]                                               (gridDim.y = 1)
// MODE BAP_COLS_GRAD: out [split][nR][D] = sum over the split's streamed rows t of wt[t] f0'(s[r, t]) Xt[t]               (raw partials)
template <int D, int MODE>
__global__ __launch_bounds__(kBlk) void bap_stream_kernel(const float *__restrict__ Xr, int nR, const float *__restrict__ Xt, int nT, int split_len,
                                                           const float *__restrict__ wt, float eps, float *__restrict__ out, float *__restrict__ rowloss) {
    constexpr int NT = D / 16;
    constexpr bool GRAD = MODE != BAP_ROWS_LOSS, LOSS = MODE != BAP_COLS_GRAD, TW = MODE == BAP_COLS_GRAD;
    __shared__ float tile[2][strm::kStageFloats<D>];
    __shared__ float tw[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(nT, t_begin + split_len);
    float br[D / 4];
    strm::load_resident<D>(Xr, r0 + c, nR, g, br);
    f32x4v o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    // second level of the weighted row sums: a stage's 64 streamed rows are summed in fp32 on the matrix cores, the stages in double (one fp32 chain
    // over all streamed rows measured 1.1e-6 against float64 at 777 rows, the staged sum 2.5e-7)
    double o2[GRAD ? NT : 1][4];
#pragma unroll
    for (int n = 0; n < (GRAD ? NT : 1); ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o2[n][reg] = 0.0;
    double rl = 0.0;
    const int nst = (t_end - t_begin + 63) / 64;
    // beside a stage's rows: the streamed rows' row_weight (BAP_COLS_GRAD), fetched and stashed with them
    strm::stage<D> stg(tid);
    float pre_w = 0.f;
#define BAP_FETCH(ST)                                                           \
    do {                                                                        \
        stg.fetch(Xt, t_begin + (ST) * 64, nT);                                 \
        if (TW && tid < 64) pre_w = wt[min(t_begin + (ST) * 64 + tid, nT - 1)]; \
    } while (0)
#define BAP_STASH(BUF)                            \
    do {                                          \
        stg.stash(tile[BUF]);                     \
        if (TW && tid < 64) tw[BUF][tid] = pre_w; \
    } while (0)
    if (nst > 0) { BAP_FETCH(0); BAP_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) BAP_FETCH(st + 1);
        const float *T = tile[buf];
        float stage_loss = 0.f;
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f32x4v sc = strm::scores<D>(strm::a_row<D>(T, sub, c, g), br);
            const int tb = t_begin + st * 64 + sub * 16 + 4 * g;        // streamed row of register 0
            float fj[4], pj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float f0, w0;
                bap_dense_terms(sc[j], eps, f0, w0);
                const bool live = tb + j < t_end;
                fj[j] = live ? f0 : 0.f;
                if (TW) w0 *= tw[buf][sub * 16 + 4 * g + j];
                pj[j] = live ? w0 : 0.f;
            }
            if (LOSS) stage_loss += (fj[0] + fj[1]) + (fj[2] + fj[3]);
            if (GRAD) strm::accumulate<D>(T, sub, c, g, pj, o);
        }
        if (LOSS) rl += (double)stage_loss;                              // 16 scores in fp32, the stages in double
        if constexpr (GRAD) strm::flush_stage<D>(o, o2);
        if (st + 1 < nst) BAP_STASH(buf ^ 1);
        __syncthreads();
    }
#undef BAP_FETCH
#undef BAP_STASH
    if (LOSS) {
        // the four lane groups of a resident row, pairwise (both lanes of a pair compute the same two-term sum)
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) rl += __shfl_xor(rl, off);
        if (g == 0 && r0 + c < nR) rowloss[r0 + c] = (float)rl;
    }
    if constexpr (GRAD) strm::store_partial<D>(out, blockIdx.y, nR, r0, g, c, o2);
}

// Pass 3, a wave per row x of the resident table X [n, D]; its listed entries k in [ptr[x], ptr[x + 1]) name rows col[k] of the other table Y and
// weights val[perm ? perm[k] : k] (val NULL: 1).  LG = D / 4 lanes hold one row as float4s; the wave's 64 / LG lane groups take the entries in turn and
// are folded in a fixed tree at the end.
//   lc  = sum_k a_k (f1 - f0)(s_k)                           -> rowloss[x] += lc                          (rowloss given: the by-user call)
//   acc = sum_k a_k wcol[col_k] (f1' - f0')(s_k) Y[col_k]    -> out[x] = upstream wrow[x] (sum over splits of part[split][x], ascending, + acc)
// part may be out itself (n_splits = 1: the by-user call finishes pass 1's raw sums in place), so neither is __restrict__.
template <int D, bool GRAD>
__global__ __launch_bounds__(kBlk) void bap_gather_kernel(const float *__restrict__ X, int n, const float *__restrict__ Y, const int32_t *__restrict__ ptr,
                                                           const int32_t *__restrict__ col, const float *__restrict__ val, const int32_t *__restrict__ perm,
                                                           const float *__restrict__ wrow, const float *__restrict__ wcol, float eps, float upstream,
                                                           const float *part, int n_splits, float *out, float *rowloss) {
#pragma clang fp contract(off)
    constexpr int LG = D / 4, G = 64 / LG;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane % LG, grp = lane / LG;
    const int x = blockIdx.x * kWaves + wv;
    if (x >= n) return;                                                  // the whole wave leaves
    const float4 xr = *reinterpret_cast<const float4 *>(X + (size_t)x * D + 4 * li);
    const int k_begin = ptr[x], k_end = ptr[x + 1];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    double lc = 0.0;
    for (int k0 = k_begin; k0 < k_end; k0 += G) {                        // the same trip count in every lane: the shuffles below see whole groups
        const int k = k0 + grp;
        const bool live = k < k_end;
        const int cidx = live ? col[k] : 0;
        const float4 y = *reinterpret_cast<const float4 *>(Y + (size_t)cidx * D + 4 * li);
        float s = fmaf(xr.w, y.w, fmaf(xr.z, y.z, fmaf(xr.y, y.y, xr.x * y.x)));
#pragma unroll
        for (int off = 1; off < LG; off <<= 1) s += __shfl_xor(s, off);
        float df, dw;
        bap_positive_terms(s, eps, df, dw);
        float a = 0.f;
        if (live) a = val ? val[perm ? perm[k] : k] : 1.0f;
        lc += (double)(a * df);
        if (GRAD) {
            float cw = a * dw;
            if (wcol) cw *= wcol[cidx];
            acc.x = fmaf(cw, y.x, acc.x); acc.y = fmaf(cw, y.y, acc.y); acc.z = fmaf(cw, y.z, acc.z); acc.w = fmaf(cw, y.w, acc.w);
        }
    }
#pragma unroll
    for (int off = LG; off < 64; off <<= 1) {
        lc += __shfl_xor(lc, off);
        if (GRAD) {
            acc.x += __shfl_xor(acc.x, off); acc.y += __shfl_xor(acc.y, off); acc.z += __shfl_xor(acc.z, off); acc.w += __shfl_xor(acc.w, off);
        }
    }
    if (grp != 0) return;
    if (rowloss && li == 0) rowloss[x] = (float)((double)rowloss[x] + lc);
    if (GRAD) {
        const size_t e = (size_t)x * D + 4 * li, stride = (size_t)n * D;
        float4 b = *reinterpret_cast<const float4 *>(part + e);
        for (int k = 1; k < n_splits; ++k) {
            const float4 b2 = *reinterpret_cast<const float4 *>(part + (size_t)k * stride + e);
            b.x += b2.x; b.y += b2.y; b.z += b2.z; b.w += b2.w;
        }
        const float sc = wrow ? upstream * wrow[x] : upstream;
        *reinterpret_cast<float4 *>(out + e) = make_float4(sc * (b.x + acc.x), sc * (b.y + acc.y), sc * (b.z + acc.z), sc * (b.w + acc.w));
    }
}

// one workgroup: loss = sum_r rw[r] rowloss[r] in double, fixed strides then a tree
__global__ __launch_bounds__(kBlk) void bap_loss_kernel(const float *__restrict__ rw, const float *__restrict__ rowloss, int n, float *__restrict__ loss) {
    __shared__ double red[kBlk];
    double v = 0.0;
    for (int r = threadIdx.x; r < n; r += kBlk) v += (double)rw[r] * (double)rowloss[r];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = (float)red[0];
}

template <int D>
int bap_run(const float *Pu, int64_t R, const float *Pi, int64_t I, const int32_t *rowptr, const int32_t *col, const float *val, const int32_t *trowptr,
            const int32_t *tcol, const int32_t *tperm, const float *rw, float eps, float upstream, float *rowloss, float *loss, float *dPu, float *dPi,
            char *ws, hipStream_t st) {
    const dim3 blk(kBlk);
    const dim3 grid_users((unsigned)((R + 63) / 64), 1u), wave_users((unsigned)((R + kWaves - 1) / kWaves)), wave_items((unsigned)((I + kWaves - 1) / kWaves));
    if (dPu) {
        hipLaunchKernelGGL((bap_stream_kernel<D, BAP_ROWS_GRAD>), grid_users, blk, 0, st, Pu, (int)R, Pi, (int)I, (int)I, (const float *)nullptr, eps, dPu, rowloss);
        ARL_LAUNCH_CHECK();
        hipLaunchKernelGGL((bap_gather_kernel<D, true>), wave_users, blk, 0, st, Pu, (int)R, Pi, rowptr, col, val, (const int32_t *)nullptr, rw, (const float *)nullptr, eps,
                           upstream, (const float *)dPu, 1, dPu, rowloss);
        ARL_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL((bap_stream_kernel<D, BAP_ROWS_LOSS>), grid_users, blk, 0, st, Pu, (int)R, Pi, (int)I, (int)I, (const float *)nullptr, eps, (float *)nullptr,
                           rowloss);
        ARL_LAUNCH_CHECK();
        hipLaunchKernelGGL((bap_gather_kernel<D, false>), wave_users, blk, 0, st, Pu, (int)R, Pi, rowptr, col, val, (const int32_t *)nullptr, rw, (const float *)nullptr, eps,
                           upstream, (const float *)nullptr, 0, (float *)nullptr, rowloss);
        ARL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bap_loss_kernel, dim3(1), blk, 0, st, rw, (const float *)rowloss, (int)R, loss);
    ARL_LAUNCH_CHECK();
    if (dPi) {
        const int ns = strm::split_count(I, R);
        const int split_len = (int)((R + ns - 1) / ns);
        float *gpart = (float *)ws;
        hipLaunchKernelGGL((bap_stream_kernel<D, BAP_COLS_GRAD>), dim3((unsigned)((I + 63) / 64), (unsigned)ns), blk, 0, st, Pi, (int)I, Pu, (int)R, split_len, rw, eps, gpart,
                           (float *)nullptr);
        ARL_LAUNCH_CHECK();
        hipLaunchKernelGGL((bap_gather_kernel<D, true>), wave_items, blk, 0, st, Pi, (int)I, Pu, trowptr, tcol, val, tperm, (const float *)nullptr, rw, eps, upstream,
                           (const float *)gpart, ns, dPi, (float *)nullptr);
        ARL_LAUNCH_CHECK();
    }
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_bce_allpairs_workspace_bytes(int64_t R, int64_t I, int64_t d, int32_t want_grad) {
    if (!strm::shape_ok(R, I, d)) return 0;
    return want_grad ? (int64_t)up16(sizeof(float) * (size_t)strm::split_count(I, R) * (size_t)I * (size_t)d) : 0;
}

int arl_bce_allpairs_f32(const float *Pu, int64_t R, const float *Pi, int64_t I, int64_t d, const int32_t *pos_rowptr, const int32_t *pos_col, const float *pos_val,
                         const int32_t *post_rowptr, const int32_t *post_col, const int32_t *post_perm, const float *row_weight, float eps, float upstream,
                         float *rowloss, float *loss, float *dPu, float *dPi, void *workspace, arl_stream_t stream) {
    if (!Pu || !Pi || !pos_rowptr || !pos_col || !row_weight || !rowloss || !loss || !workspace) return ARL_E_NULL;
    if (dPi && (!post_rowptr || !post_col || (pos_val && !post_perm))) return ARL_E_NULL;
    if (d != 16 && d != 32 && d != 64 && d != 128) return ARL_E_DIM;
    if (R <= 0 || I <= 0 || !(eps >= 0.f)) return ARL_E_ARG;
    if (R > 0x7fffffffll / 128 || I > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)Pu | (uintptr_t)Pi | (uintptr_t)dPu | (uintptr_t)dPi | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define BAP_RUN(DD) return bap_run<DD>(Pu, R, Pi, I, pos_rowptr, pos_col, pos_val, post_rowptr, post_col, post_perm, row_weight, eps, upstream, rowloss, loss, dPu, dPi, ws, st)
    ARL_DISPATCH_WIDTH(d, BAP_RUN);
#undef BAP_RUN
}

}  // extern "C"

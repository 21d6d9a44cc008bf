// arl_colsoftmax.hip -- LegUP's ranking loss L_RS (reference attack/Gray/LegUP.py:160-171) on gfx950 without the U x I score matrix.
//
// With s = Pu Pi^T [U, I], target columns c_0 .. c_{T-1} and lse[i] = log sum_u exp(s[u, i]) (a softmax over the USERS of every item column),
// the reference's broadcast  -sum(log(exp(s[:, c])[:, :, None] / sum_u exp(s)))  over [U, T, I]  is
//     L = -( I * sum_u sum_t s[u, c_t]  -  U * T * sum_i lse[i] ),
//     dL/ds[u, i] = U T P[u, i] - I #{t : c_t = i},       P[u, i] = exp(s[u, i] - lse[i]),
//     dPu[u] = U T sum_i P[u, i] Pi[i] - I sum_t Pi[c_t],   dPi[i] = U T sum_u P[u, i] Pu[u] - I #{t : c_t = i} sum_u Pu[u].
//
// Rules kept throughout:
//   * scores and the P-weighted row sums run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h);
//   * three passes: lse (items resident, users streamed in splits, running maximum), dPi (items resident, users streamed in splits), dPu (users
//     resident, all items streamed, one writer per output row);
//   * every reduction has a fixed order (lane groups, then splits / row chunks ascending): no atomics, bit-identical from run to run;
//   * sum_u s[u, c_t] is <sum_u Pu[u], Pi[c_t]>: the column sum of Pu and the scalar sums are accumulated in double.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr float kNegBig = -3.0e38f;          // running maximum before any score (finite: exp(kNegBig - m) is 0, never NaN)
using strm::f32x4v;

enum { CSM_LSE = 0, CSM_GRAD_LSE_R = 1, CSM_GRAD_LSE_T = 2 };

// MODE CSM_LSE       : pm / ps [split][nR] = running maximum and sum of exp(s - maximum) of resident row r over the split's streamed rows
// MODE CSM_GRAD_LSE_R: out [split][nR][D] = sum_t exp(s[t, r] - lse[r]) Xt[t]          (lse belongs to the resident rows; raw partials)
// MODE CSM_GRAD_LSE_T: out [nR][D] = scale * sum_t exp(s[t, r] - lse[t]) Xt[t] - sub    (lse belongs to the streamed rows; gridDim.y = 1)
template <int D, int MODE>
__global__ __launch_bounds__(kBlk) void csm_stream_kernel(const float *__restrict__ Xr, int nR, const float *__restrict__ Xt, int nT, int split_len,
                                                           const float *__restrict__ lse, float scale, const float *__restrict__ sub_vec,
                                                           float *__restrict__ out, float *__restrict__ pm, float *__restrict__ ps) {
    constexpr int NT = D / 16;
    constexpr bool GRAD = MODE != CSM_LSE;
    __shared__ float tile[2][strm::kStageFloats<D>];
    __shared__ float tlse[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(nT, t_begin + split_len);
    float br[D / 4];
    strm::load_resident<D>(Xr, r0 + c, nR, g, br);
    const float lse_r = (MODE == CSM_GRAD_LSE_R && r0 + c < nR) ? lse[r0 + c] : 0.f;
    f32x4v o[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) o[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    float m = kNegBig, sum = 0.f;
    const int nst = (t_end - t_begin + 63) / 64;
    // beside a stage's rows: the streamed rows' lse (CSM_GRAD_LSE_T), fetched and stashed with them
    strm::stage<D> stg(tid);
    float pre_lse = 0.f;
#define CSM_FETCH(ST)                                                                                  \
    do {                                                                                               \
        stg.fetch(Xt, t_begin + (ST) * 64, nT);                                                        \
        if (MODE == CSM_GRAD_LSE_T && tid < 64) pre_lse = lse[min(t_begin + (ST) * 64 + tid, nT - 1)]; \
    } while (0)
#define CSM_STASH(BUF)                                                    \
    do {                                                                  \
        stg.stash(tile[BUF]);                                             \
        if (MODE == CSM_GRAD_LSE_T && tid < 64) tlse[BUF][tid] = pre_lse; \
    } while (0)
    if (nst > 0) { CSM_FETCH(0); CSM_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) CSM_FETCH(st + 1);
        const float *T = tile[buf];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const f32x4v sc = strm::scores<D>(strm::a_row<D>(T, sub, c, g), br);
            const int tb = t_begin + st * 64 + sub * 16 + 4 * g;        // streamed row of register 0
            if (!GRAD) {
                float mx = m;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (tb + j < t_end) mx = fmaxf(mx, sc[j]);
                if (mx > m) { sum *= expf(m - mx); m = mx; }
                float e[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) e[j] = tb + j < t_end ? expf(sc[j] - m) : 0.f;
                sum += (e[0] + e[1]) + (e[2] + e[3]);
            } else {
                float pj[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float l = MODE == CSM_GRAD_LSE_R ? lse_r : tlse[buf][sub * 16 + 4 * g + j];
                    pj[j] = tb + j < t_end ? expf(sc[j] - l) : 0.f;
                }
                strm::accumulate<D>(T, sub, c, g, pj, o);
            }
        }
        if (st + 1 < nst) CSM_STASH(buf ^ 1);
        __syncthreads();
    }
#undef CSM_FETCH
#undef CSM_STASH
    if (!GRAD) {
        // the four lane groups of a resident row, pairwise (both lanes of a pair compute the same two-term sum)
#pragma unroll
        for (int off = 16; off <= 32; off <<= 1) {
            const float m2 = __shfl_xor(m, off), s2 = __shfl_xor(sum, off);
            const float mm = fmaxf(m, m2);
            const float a = sum * expf(m - mm), b = s2 * expf(m2 - mm);
            sum = (lane & off) ? b + a : a + b;
            m = mm;
        }
        if (g == 0 && r0 + c < nR) {
            pm[(size_t)blockIdx.y * nR + r0 + c] = m;
            ps[(size_t)blockIdx.y * nR + r0 + c] = sum;
        }
    } else if (MODE == CSM_GRAD_LSE_R) {
        strm::store_partial<D>(out, blockIdx.y, nR, r0, g, c, o);
    } else {
#pragma unroll
        for (int n = 0; n < NT; ++n)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int r = r0 + 4 * g + reg;
                if (r < nR) out[(size_t)r * D + 16 * n + c] = scale * o[n][reg] - sub_vec[16 * n + c];
            }
    }
}

// column sums of X [n, d] in double over fixed row chunks: part[b][k] = sum of rows [b * chunk, (b + 1) * chunk) of column k
__global__ __launch_bounds__(kBlk) void csm_colsum_partial_kernel(const float *__restrict__ X, long long n, int d, long long chunk, double *__restrict__ part) {
    __shared__ double red[kBlk];
    const int k = threadIdx.x % d, lanes = kBlk / d, rl = threadIdx.x / d;
    const long long r_begin = (long long)blockIdx.x * chunk, r_end = min(n, r_begin + chunk);
    double s = 0.0;
    for (long long r = r_begin + rl; r < r_end; r += lanes) s += (double)X[r * d + k];
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
        for (int j = 1; j < lanes; ++j) s += red[j * d + k];
        part[(size_t)blockIdx.x * d + k] = s;
    }
}

// one workgroup: usum[k] = sum of the chunks in order; tsum[k] = sum_t Pi[c_t][k]; head[0] = sum_t <usum, Pi[c_t]>;
// sub_u[k] = I * tsum[k] (what dPu subtracts), sub_i[k] = I * usum[k] (what dPi subtracts per listed target)
__global__ __launch_bounds__(kBlk) void csm_head_kernel(const double *__restrict__ part, int n_chunks, const float *__restrict__ Pi, const int32_t *__restrict__ targets,
                                                         int T, int d, double n_items, double *__restrict__ head, float *__restrict__ sub_u, float *__restrict__ sub_i) {
    __shared__ double prod[128];
    const int k = threadIdx.x;
    if (k < d) {
        double u = 0.0, t = 0.0;
        for (int b = 0; b < n_chunks; ++b) u += part[(size_t)b * d + k];
        for (int j = 0; j < T; ++j) t += (double)Pi[(size_t)targets[j] * d + k];
        prod[k] = u * t;
        sub_u[k] = (float)(n_items * t);
        sub_i[k] = (float)(n_items * u);
    }
    __syncthreads();
    if (k == 0) {
        double a = 0.0;
        for (int j = 0; j < d; ++j) a += prod[j];
        head[0] = a;
    }
}

// lse[i] = M + log(sum over splits of ps * exp(pm - M)), M = the largest pm, splits in order; lpart[block] = sum of the block's lse in double
__global__ __launch_bounds__(kBlk) void csm_lse_finish_kernel(const float *__restrict__ pm, const float *__restrict__ ps, int n_splits, int nI, float *__restrict__ lse,
                                                               double *__restrict__ lpart) {
    __shared__ double red[kBlk];
    const int i = blockIdx.x * kBlk + threadIdx.x;
    double v = 0.0;
    if (i < nI) {
        float M = pm[i];
        for (int k = 1; k < n_splits; ++k) M = fmaxf(M, pm[(size_t)k * nI + i]);
        float s = 0.f;
        for (int k = 0; k < n_splits; ++k) s += ps[(size_t)k * nI + i] * expf(pm[(size_t)k * nI + i] - M);
        const float l = M + logf(s);
        lse[i] = l;
        v = (double)l;
    }
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) lpart[blockIdx.x] = red[0];
}

// one workgroup: loss = -(I * head[0] - U * T * sum of lpart), lpart folded by fixed strides then a tree
__global__ __launch_bounds__(kBlk) void csm_loss_kernel(const double *__restrict__ head, const double *__restrict__ lpart, int n_part, double n_users, double n_items,
                                                         double n_targets, float *__restrict__ loss) {
    __shared__ double red[kBlk];
    double v = 0.0;
    for (int b = threadIdx.x; b < n_part; b += kBlk) v += lpart[b];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = (float)(-(n_items * head[0] - n_users * n_targets * red[0]));
}

// dPi[i][:] = scale * (sum over splits of part, in order) - (number of t with c_t = i) * sub_i
__global__ __launch_bounds__(kBlk) void csm_fold_items_kernel(const float4 *__restrict__ part, int n_splits, int nI, int d4, float scale, const int32_t *__restrict__ targets,
                                                               int T, const float *__restrict__ sub_i, float4 *__restrict__ out) {
    const long long n4 = (long long)nI * d4;
    for (long long e = (long long)blockIdx.x * kBlk + threadIdx.x; e < n4; e += (long long)gridDim.x * kBlk) {
        const int i = (int)(e / d4), q = (int)(e - (long long)i * d4);
        float4 a = part[e];
        for (int k = 1; k < n_splits; ++k) {
            const float4 b = part[(size_t)k * n4 + e];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        int cnt = 0;
        for (int t = 0; t < T; ++t) cnt += targets[t] == i;
        const float cf = (float)cnt;
        const float4 s = *reinterpret_cast<const float4 *>(sub_i + 4 * q);
        out[e] = make_float4(scale * a.x - cf * s.x, scale * a.y - cf * s.y, scale * a.z - cf * s.z, scale * a.w - cf * s.w);
    }
}

int csm_chunks(int64_t U) {
    const int64_t c = (U + 1023) / 1024;
    return (int)(c > 1024 ? 1024 : (c < 1 ? 1 : c));
}

struct CsmLayout {
    size_t colpart, head, lpart, sub_u, sub_i, pm, ps, gpart, total;
    int ns, chunks, lblocks;
};

CsmLayout csm_layout(int64_t U, int64_t I, int64_t d, bool want_dPi) {
    CsmLayout L;
    L.ns = strm::split_count(I, U);
    L.chunks = csm_chunks(U);
    L.lblocks = (int)((I + kBlk - 1) / kBlk);
    size_t o = 0;
    L.colpart = o; o = up16(o + sizeof(double) * (size_t)L.chunks * d);
    L.head = o;    o = up16(o + sizeof(double) * 2);
    L.lpart = o;   o = up16(o + sizeof(double) * (size_t)L.lblocks);
    L.sub_u = o;   o = up16(o + sizeof(float) * d);
    L.sub_i = o;   o = up16(o + sizeof(float) * d);
    L.pm = o;      o = up16(o + sizeof(float) * (size_t)L.ns * I);
    L.ps = o;      o = up16(o + sizeof(float) * (size_t)L.ns * I);
    L.gpart = o;   if (want_dPi) o = up16(o + sizeof(float) * (size_t)L.ns * I * d);
    L.total = o;
    return L;
}

template <int D>
int csm_run(const float *Pu, int64_t U, const float *Pi, int64_t I, const int32_t *targets, int64_t T, float *lse, float *loss, float *dPu, float *dPi,
            char *ws, hipStream_t st) {
    const CsmLayout L = csm_layout(U, I, D, dPi != nullptr);
    double *colpart = (double *)(ws + L.colpart), *head = (double *)(ws + L.head), *lpart = (double *)(ws + L.lpart);
    float *sub_u = (float *)(ws + L.sub_u), *sub_i = (float *)(ws + L.sub_i), *pm = (float *)(ws + L.pm), *ps = (float *)(ws + L.ps);
    float *gpart = (float *)(ws + L.gpart);
    const long long chunk = (U + L.chunks - 1) / L.chunks;
    hipLaunchKernelGGL(csm_colsum_partial_kernel, dim3((unsigned)L.chunks), dim3(kBlk), 0, st, Pu, (long long)U, D, chunk, colpart);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csm_head_kernel, dim3(1), dim3(kBlk), 0, st, colpart, L.chunks, Pi, targets, (int)T, D, (double)I, head, sub_u, sub_i);
    ARL_LAUNCH_CHECK();
    const int split_len = (int)((U + L.ns - 1) / L.ns);
    const dim3 grid_items((unsigned)((I + 63) / 64), (unsigned)L.ns);
    hipLaunchKernelGGL((csm_stream_kernel<D, CSM_LSE>), grid_items, dim3(kBlk), 0, st, Pi, (int)I, Pu, (int)U, split_len, (const float *)nullptr, 0.f,
                       (const float *)nullptr, (float *)nullptr, pm, ps);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csm_lse_finish_kernel, dim3((unsigned)L.lblocks), dim3(kBlk), 0, st, pm, ps, L.ns, (int)I, lse, lpart);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(csm_loss_kernel, dim3(1), dim3(kBlk), 0, st, head, lpart, L.lblocks, (double)U, (double)I, (double)T, loss);
    ARL_LAUNCH_CHECK();
    const float scale = (float)((double)U * (double)T);
    if (dPi) {
        hipLaunchKernelGGL((csm_stream_kernel<D, CSM_GRAD_LSE_R>), grid_items, dim3(kBlk), 0, st, Pi, (int)I, Pu, (int)U, split_len, (const float *)lse, 0.f,
                           (const float *)nullptr, gpart, (float *)nullptr, (float *)nullptr);
        ARL_LAUNCH_CHECK();
        const long long n4 = I * (D / 4);
        long long blocks = (n4 + kBlk - 1) / kBlk;
        if (blocks > 65535) blocks = 65535;
        hipLaunchKernelGGL(csm_fold_items_kernel, dim3((unsigned)blocks), dim3(kBlk), 0, st, (const float4 *)gpart, L.ns, (int)I, D / 4, scale, targets, (int)T,
                           (const float *)sub_i, (float4 *)dPi);
        ARL_LAUNCH_CHECK();
    }
    if (dPu) {
        hipLaunchKernelGGL((csm_stream_kernel<D, CSM_GRAD_LSE_T>), dim3((unsigned)((U + 63) / 64), 1u), dim3(kBlk), 0, st, Pu, (int)U, Pi, (int)I, (int)I,
                           (const float *)lse, scale, (const float *)sub_u, dPu, (float *)nullptr, (float *)nullptr);
        ARL_LAUNCH_CHECK();
    }
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_colsoftmax_target_workspace_bytes(int64_t U, int64_t I, int64_t d, int32_t want_dPi) {
    if (U <= 0 || I <= 0 || (d != 16 && d != 32 && d != 64 && d != 128)) return 0;
    return (int64_t)csm_layout(U, I, d, want_dPi != 0).total;
}

int arl_colsoftmax_target_loss_f32(const float *Pu, int64_t U, const float *Pi, int64_t I, int64_t d, const int32_t *targets, int64_t T, float *lse, float *loss,
                                   float *dPu, float *dPi, void *workspace, arl_stream_t stream) {
    if (!Pu || !Pi || !targets || !lse || !loss || !workspace) return ARL_E_NULL;
    if (d != 16 && d != 32 && d != 64 && d != 128) return ARL_E_DIM;
    if (U <= 0 || I <= 0 || T <= 0 || T > 1024) return ARL_E_ARG;
    if (U > 0x7fffffffll / 128 || I > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)Pu | (uintptr_t)Pi | (uintptr_t)dPu | (uintptr_t)dPi | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define CSM_RUN(DD) return csm_run<DD>(Pu, U, Pi, I, targets, T, lse, loss, dPu, dPi, ws, st)
    ARL_DISPATCH_WIDTH(d, CSM_RUN);
#undef CSM_RUN
}

}  // extern "C"

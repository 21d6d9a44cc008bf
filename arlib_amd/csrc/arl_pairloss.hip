// arl_pairloss.hip -- the two terms of DirectAU (reference util/loss.py:17-23: alignment_loss, uniformity_loss) on gfx950, forward and backward.
//
// Uniformity of raw rows X [n, d]:  y = F.normalize(x),  loss = log( mean_{i<j} exp(-t |y_i - y_j|^2) ).  The reference stores all n (n - 1) / 2
// distances (torch.pdist); here none is stored.  Rules kept throughout:
//   * dist^2_ij = max(q_i + q_j - 2 <y_i, y_j>, 0) with q_r = |y_r|^2 kept per row: rows are NOT assumed to have unit length (F.normalize leaves a
//     zero row at zero and scales a row of norm < 1e-12 by 1e12);
//   * products run exact fp32 on v_mfma_f32_16x16x4_f32 on the shared streamed tile (arl_stream.h), the streamed rows' q beside each stage;
//     e = exp(-t dist^2) of the score tile is already in A-operand layout for the second product G_i = sum_j e_ij y_j, which runs here on
//     v_mfma_f64_16x16x4_f64 (same operand layout; result register reg of lane (c, g) is row g + 4 reg, not 4 g + reg);
//   * the diagonal is masked (e_ii never enters a sum), rows past a split's end likewise; the plain both-orders sweep, no triangle skipped;
//   * every sum has a fixed order (no float atomics): a lane's four scores, the stage's four tiles, the four lane groups by two butterflies, the
//     splits of the streamed side in split order, S = sum_i rowsum_i in double over fixed spans (arl_kmeans_sum_f64);
//   * loss = log(S / (n (n - 1))),  dL/dy_i = (-4 t / S) (y_i rowsum_i - G_i),  then the autograd of the normalisation with the upstream gradient;
//   * y_i rowsum_i - G_i cancels (rows of one cluster: thirteen-fold at four clusters, and the normalisation's backward then removes the radial
//     part of what is left), so a rounding error of rowsum or G relative to ITS size is that much larger relative to the gradient, and the
//     reference's pdist, which subtracts the rows first, has no such loss.  So rowsum and G are summed in double from the first term on (the
//     products e y are exact in double), and the difference is formed in double and rounded once to fp32.
//
// Alignment of raw rows X, Y [n, d]:  mean_b |x^_b - y^_b|^alpha, one wave per row pair, gradients for both inputs; a pair with x^_b == y^_b
// contributes gradient 0 (torch's subgradient of the norm at the origin).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr int kSplitRows = 256;              // a split of the streamed side has at least this many rows
using strm::f32x4v;
typedef double f64x4v __attribute__((ext_vector_type(4)));

// q[r] = |Y[r]|^2, one thread per row, components in order
__global__ __launch_bounds__(kBlk) void unif_q_kernel(const float *__restrict__ Y, int n, int d, float *__restrict__ q) {
    const int r = blockIdx.x * kBlk + threadIdx.x;
    if (r >= n) return;
    const float4 *row = reinterpret_cast<const float4 *>(Y + (size_t)r * d);
    float s = 0.f;
    for (int k = 0; k < d / 4; ++k) {
        const float4 v = row[k];
        s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
    }
    q[r] = s;
}

// For the resident rows r of this workgroup and the streamed rows j of split blockIdx.y, j != r, with e = exp(neg_t * max(q_r + q_j - 2 <y_r, y_j>, 0)):
//   sums[split][r] = sum_j e,   GRAD: part[split][r][:] = y_r sum_j e - sum_j e y_j.
template <int D, bool GRAD>
__global__ __launch_bounds__(kBlk) void unif_pairs_kernel(const float *__restrict__ Y, const float *__restrict__ q, int n, int split_len, float neg_t,
                                                           float *__restrict__ part, float *__restrict__ sums) {
    constexpr int LD = strm::kLD<D>, NT = D / 16;
    __shared__ __attribute__((aligned(16))) float tile[2][strm::kStageFloats<D>];
    __shared__ __attribute__((aligned(16))) float tq[2][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(n, t_begin + split_len);
    float br[D / 4];
    strm::load_resident<D>(Y, r0 + c, n, g, br);
    const float q_r = r0 + c < n ? q[r0 + c] : 0.f;
    f64x4v od[NT];                           // G's tile and the row sums, in double
#pragma unroll
    for (int m = 0; m < NT; ++m) od[m] = f64x4v{0.0, 0.0, 0.0, 0.0};
    double sumd = 0.0;
    const int nst = t_end > t_begin ? (t_end - t_begin + 63) / 64 : 0;
    // beside a stage's rows: their q, fetched and stashed with them
    strm::stage<D> stg(tid);
    float pre_q = 0.f;
#define PL_FETCH(ST)                                                    \
    do {                                                                \
        stg.fetch(Y, t_begin + (ST) * 64, n);                           \
        if (tid < 64) pre_q = q[min(t_begin + (ST) * 64 + tid, n - 1)]; \
    } while (0)
#define PL_STASH(BUF)                       \
    do {                                    \
        stg.stash(tile[BUF]);               \
        if (tid < 64) tq[BUF][tid] = pre_q; \
    } while (0)
    if (nst > 0) { PL_FETCH(0); PL_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) PL_FETCH(st + 1);
        const float *T = tile[buf];
        // the stage's four 16-row tiles on four independent accumulators: strm::scores4, written out (through the helper the gradient form at
        // d = 64 moves 14 registers to the AGPR side and loses a wave of occupancy)
        f32x4v sc[4];
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) sc[sub] = f32x4v{0.f, 0.f, 0.f, 0.f};
        const float *arow = strm::a_row<D>(T, 0, c, g);
#pragma unroll
        for (int i = 0; i < D / 4; i += 4) {
            float4 a[4];
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) a[sub] = *reinterpret_cast<const float4 *>(arow + sub * 16 * LD + i);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].x, br[i], sc[sub], 0, 0, 0);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].y, br[i + 1], sc[sub], 0, 0, 0);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].z, br[i + 2], sc[sub], 0, 0, 0);
#pragma unroll
            for (int sub = 0; sub < 4; ++sub) sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].w, br[i + 3], sc[sub], 0, 0, 0);
        }
        // register j of tile sub is streamed row tb + j against resident row r0 + c
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            const int tl = sub * 16 + 4 * g, tb = t_begin + st * 64 + tl;
            const float4 q4 = *reinterpret_cast<const float4 *>(&tq[buf][tl]);
            const float qj[4] = {q4.x, q4.y, q4.z, q4.w};
            float pj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float d2 = fmaxf((q_r + qj[j]) - 2.f * sc[sub][j], 0.f);
                pj[j] = (tb + j < t_end && tb + j != r0 + c) ? expf(neg_t * d2) : 0.f;
            }
            sumd += ((double)pj[0] + (double)pj[1]) + ((double)pj[2] + (double)pj[3]);
            if (GRAD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float *brow = T + (tl + j) * LD + c;
                    const double pd = (double)pj[j];
#pragma unroll
                    for (int m = 0; m < NT; ++m) od[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(pd, (double)brow[16 * m], od[m], 0, 0, 0);
                }
            }
        }
        if (st + 1 < nst) PL_STASH(buf ^ 1);
        __syncthreads();
    }
#undef PL_FETCH
#undef PL_STASH
    sumd += __shfl_xor(sumd, 16); sumd += __shfl_xor(sumd, 32);         // over the four lane groups (fixed order): every lane of row c has the row's sum
    if (g == 0 && r0 + c < n) sums[(size_t)blockIdx.y * n + r0 + c] = (float)sumd;
    if (GRAD) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = r0 + g + 4 * reg;                             // the f64 form's result rows
            const double rs = __shfl(sumd, g + 4 * reg);                // lane g + 4 reg holds row r0 + g + 4 reg
            if (r < n) {
#pragma unroll
                for (int m = 0; m < NT; ++m) {
                    const size_t at = (size_t)r * D + 16 * m + c;
                    part[(size_t)blockIdx.y * n * D + at] = (float)((double)Y[at] * rs - od[m][reg]);
                }
            }
        }
    }
}

// rowsum[i] = the splits' partial sums in split order
__global__ __launch_bounds__(kBlk) void unif_rowsum_kernel(const float *__restrict__ sums, int n_splits, int n, float *__restrict__ rowsum) {
    const int i = blockIdx.x * kBlk + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int k = 0; k < n_splits; ++k) s += sums[(size_t)k * n + i];
    rowsum[i] = s;
}

// loss = log(S / (n (n - 1)));  dYn[i][:] = (-4 t / S) (sum over splits of part[k][i][:]), splits in order (part == NULL: the loss alone)
__global__ __launch_bounds__(kBlk) void unif_finish_kernel(const double *__restrict__ S, float t, int n, int d4, const float4 *__restrict__ part, int n_splits,
                                                            float *__restrict__ loss, float4 *__restrict__ dYn) {
    const double s = S[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) loss[0] = (float)log(s / ((double)n * (double)(n - 1)));
    if (!part) return;
    const float coef = (float)(-4.0 * (double)t / s);
    const long long n4 = (long long)n * d4;
    for (long long i = (long long)blockIdx.x * kBlk + threadIdx.x; i < n4; i += (long long)gridDim.x * kBlk) {
        float4 a = part[i];
        for (int k = 1; k < n_splits; ++k) {
            const float4 b = part[(size_t)k * n4 + i];
            a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
        }
        dYn[i] = make_float4(coef * a.x, coef * a.y, coef * a.z, coef * a.w);
    }
}

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ inline float dot4(const float4 a, const float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }

// One wave per row pair, lane l holds columns [4 l, 4 l + 4).  terms[b] = |x^ - y^|^alpha;  with dX: the gradients of coef_n * sum_b terms[b]
// (coef_n = upstream / n) through both normalisations; a row at the 1e-12 clamp passes its gradient divided by the clamp, as torch's clamp_min.
__global__ __launch_bounds__(kBlk) void align_rows_kernel(const float *__restrict__ X, const float *__restrict__ Y, long long n, int d, float alpha, float coef_n,
                                                           float *__restrict__ terms, float *__restrict__ dX, float *__restrict__ dY) {
    const int lane = threadIdx.x & 63;
    const bool live = lane * 4 < d;
    for (long long b = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6); b < n; b += (long long)gridDim.x * kWaves) {
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f), y = x;
        if (live) {
            x = *reinterpret_cast<const float4 *>(X + b * d + lane * 4);
            y = *reinterpret_cast<const float4 *>(Y + b * d + lane * 4);
        }
        const float nx = fmaxf(sqrtf(wave_sum(dot4(x, x))), 1e-12f), ny = fmaxf(sqrtf(wave_sum(dot4(y, y))), 1e-12f);
        const float4 xh = make_float4(x.x / nx, x.y / nx, x.z / nx, x.w / nx), yh = make_float4(y.x / ny, y.y / ny, y.z / ny, y.w / ny);
        const float4 e = make_float4(xh.x - yh.x, xh.y - yh.y, xh.z - yh.z, xh.w - yh.w);
        const float dn = sqrtf(wave_sum(dot4(e, e)));
        if (lane == 0) terms[b] = powf(dn, alpha);
        if (!dX) continue;
        const float w = dn > 0.f ? coef_n * alpha * powf(dn, alpha - 2.f) : 0.f;       // d |e|^alpha / de = alpha |e|^(alpha - 2) e, 0 at the origin
        const float4 gx = make_float4(w * e.x, w * e.y, w * e.z, w * e.w);
        const float px = wave_sum(dot4(xh, gx)), py = -wave_sum(dot4(yh, gx));
        const float dotx = nx > 1e-12f ? px : 0.f, doty = ny > 1e-12f ? py : 0.f;
        if (live) {
            *reinterpret_cast<float4 *>(dX + b * d + lane * 4) =
                make_float4((gx.x - xh.x * dotx) / nx, (gx.y - xh.y * dotx) / nx, (gx.z - xh.z * dotx) / nx, (gx.w - xh.w * dotx) / nx);
            *reinterpret_cast<float4 *>(dY + b * d + lane * 4) =
                make_float4((-gx.x - yh.x * doty) / ny, (-gx.y - yh.y * doty) / ny, (-gx.z - yh.z * doty) / ny, (-gx.w - yh.w * doty) / ny);
        }
    }
}

// loss = (sum of terms in double: a thread's strided elements, then a tree over the one workgroup) / n
__global__ __launch_bounds__(kBlk) void align_mean_kernel(const float *__restrict__ terms, long long n, float *__restrict__ loss) {
    __shared__ double red[kBlk];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += kBlk) s += (double)terms[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlk / 2; w > 0; w >>= 1) { if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w]; __syncthreads(); }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] / (double)n);
}

bool pl_rows(int64_t n) { return n >= 2 && n <= 0x7fffffffll / 128; }

// splits of the streamed side: enough workgroups to fill the chip several times over, at least kSplitRows streamed rows each
int unif_splits(int64_t n) {
    const int64_t row_blocks = (n + 63) / 64;
    int64_t s = (2048 + row_blocks - 1) / row_blocks;
    const int64_t max_s = (n + kSplitRows - 1) / kSplitRows;
    if (s > max_s) s = max_s;
    if (s > 512) s = 512;
    return (int)(s < 1 ? 1 : s);
}

inline int64_t pad16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// the workspace: Y [n][d] | dYn [n][d] | part [splits][n][d] | sums [splits][n] | nrm [n] | q [n] | rowsum [n] | S [2] double | the double sum's spans
struct UnifWs {
    float *Y, *dYn, *part, *sums, *nrm, *q, *rowsum;
    double *S;
    void *sum_ws;
    int64_t bytes;
};

UnifWs unif_ws(void *base, int64_t n, int64_t d, int ns) {
    UnifWs w;
    char *p = (char *)base;
    const int64_t tab = pad16((int64_t)sizeof(float) * n * d), vec = pad16((int64_t)sizeof(float) * n);
    w.Y = (float *)p; p += tab;
    w.dYn = (float *)p; p += tab;
    w.part = (float *)p; p += tab * ns;
    w.sums = (float *)p; p += pad16((int64_t)sizeof(float) * n * ns);
    w.nrm = (float *)p; p += vec;
    w.q = (float *)p; p += vec;
    w.rowsum = (float *)p; p += vec;
    w.S = (double *)p; p += 16;
    w.sum_ws = p; p += pad16(arl_kmeans_sum_workspace_bytes());
    w.bytes = p - (char *)base;
    return w;
}

template <int D>
int unif_pairs_run(const UnifWs &w, int64_t n, int ns, float t, bool grad, hipStream_t st) {
    const int split_len = (int)((n + ns - 1) / ns);
    const dim3 grid((unsigned)((n + 63) / 64), (unsigned)ns);
    if (grad) hipLaunchKernelGGL((unif_pairs_kernel<D, true>), grid, dim3(kBlk), 0, st, (const float *)w.Y, (const float *)w.q, (int)n, split_len, -t, w.part, w.sums);
    else hipLaunchKernelGGL((unif_pairs_kernel<D, false>), grid, dim3(kBlk), 0, st, (const float *)w.Y, (const float *)w.q, (int)n, split_len, -t, w.part, w.sums);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_uniformity_splits(int64_t n) { return pl_rows(n) ? unif_splits(n) : 0; }

int64_t arl_uniformity_workspace_bytes(int64_t n, int64_t d) {
    if (!pl_rows(n) || !arl_width_ok(d)) return 0;
    return unif_ws(nullptr, n, d, unif_splits(n)).bytes;
}

int arl_uniformity_fwd_bwd_f32(const float *X, int64_t n, int64_t d, float t, float upstream, float *loss, float *dX, void *workspace, arl_stream_t stream) {
    if (!X || !loss || !workspace) return ARL_E_NULL;
    if (!arl_width_ok(d)) return ARL_E_DIM;
    if (n < 2 || !(t > 0.f)) return ARL_E_ARG;
    if (!pl_rows(n)) return ARL_E_RANGE;
    if (((uintptr_t)X | (uintptr_t)dX | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ns = unif_splits(n);
    const UnifWs w = unif_ws(workspace, n, d, ns);
    const bool grad = dX != nullptr;
    int rc = arl_normalize_rows_f32(X, n, d, w.Y, w.nrm, stream);
    if (rc != ARL_OK) return rc;
    hipLaunchKernelGGL(unif_q_kernel, dim3((unsigned)((n + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const float *)w.Y, (int)n, (int)d, w.q);
    ARL_LAUNCH_CHECK();
    if (d == 16) rc = unif_pairs_run<16>(w, n, ns, t, grad, st);
    else if (d == 32) rc = unif_pairs_run<32>(w, n, ns, t, grad, st);
    else if (d == 64) rc = unif_pairs_run<64>(w, n, ns, t, grad, st);
    else rc = unif_pairs_run<128>(w, n, ns, t, grad, st);
    if (rc != ARL_OK) return rc;
    hipLaunchKernelGGL(unif_rowsum_kernel, dim3((unsigned)((n + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const float *)w.sums, ns, (int)n, w.rowsum);
    ARL_LAUNCH_CHECK();
    rc = arl_kmeans_sum_f64(w.rowsum, n, 0, w.S, w.sum_ws, stream);
    if (rc != ARL_OK) return rc;
    const long long n4 = (long long)n * (d / 4), blocks = (n4 + kBlk - 1) / kBlk;
    hipLaunchKernelGGL(unif_finish_kernel, dim3(grad ? (unsigned)(blocks < 16384 ? blocks : 16384) : 1u), dim3(kBlk), 0, st, (const double *)w.S, t, (int)n, (int)(d / 4),
                       grad ? (const float4 *)w.part : (const float4 *)nullptr, ns, loss, (float4 *)w.dYn);
    ARL_LAUNCH_CHECK();
    if (!grad) return ARL_OK;
    return arl_normalize_rows_bwd_f32(w.Y, w.nrm, w.dYn, n, d, upstream, nullptr, dX, stream);
}

int arl_alignment_fwd_bwd_f32(const float *X, const float *Y, int64_t n, int64_t d, float alpha, float upstream, float *loss, float *dX, float *dY, float *terms,
                              arl_stream_t stream) {
    if (!X || !Y || !loss || !terms) return ARL_E_NULL;
    if ((dX == nullptr) != (dY == nullptr)) return ARL_E_ARG;
    if (d <= 0 || d > 256 || (d & 3)) return ARL_E_DIM;
    if (n < 1 || !(alpha > 0.f)) return ARL_E_ARG;
    if (n > 0x7fffffffll / 128) return ARL_E_RANGE;
    if (((uintptr_t)X | (uintptr_t)Y | (uintptr_t)dX | (uintptr_t)dY) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const long long blocks = (n + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(align_rows_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kBlk), 0, st, X, Y, (long long)n, (int)d, alpha,
                       (float)((double)upstream / (double)n), terms, dX, dY);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(align_mean_kernel, dim3(1), dim3(kBlk), 0, st, (const float *)terms, (long long)n, loss);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

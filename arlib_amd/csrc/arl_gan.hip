// arl_gan.hip -- gfx950 kernels of AUSH's GAN (reference attack/Gray/AUSH.py): the template build, the generator's dense products on the
// matrix cores, its sparse first layer, the per-row loss partials, the fixed-order reductions and the threshold compaction.
//
//   G: Y = sigmoid(relu(T W1^T + b1) W2^T + b2) over the F x S template T (sparse, S = I // 5 + T selected items);  D: sigmoid(x w_D + b_D).
//
// Rules kept throughout:
//   * the dense products run exact fp32 on v_mfma_f32_16x16x4_f32, one workgroup per 128 x 128 output tile over the whole K range: no
//     split-K, no float atomics, so every result is bit-identical from run to run;
//   * sparse products gather rows of a row-major operand in the CSR order of their row (the template's CSR for layer 1, its CSC for dW1);
//   * column sums fold fixed row chunks, then the chunks in ascending order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_util.h"

namespace {

constexpr int kBlk = 256;
typedef float f32x4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------ dense products
// C[m, n] = sum_k A(m, k) B(k, n), A(m, k) = A[m * sam + k * sak], B(k, n) = B[k * sbk + n * sbn].  A_KC: A contiguous along k (else along m);
// B_NC: B contiguous along n (else along k).  128 x 128 tile per workgroup, 4 waves of 64 x 64 (4 x 4 MFMA tiles), K in slices of 16 staged in LDS.
// GPAD = 16: the operand reads As[ks + q][wm + 16 t + c] of a wave land on banks 16 q + c (row stride 144 floats), all 64 distinct
constexpr int GBM = 128, GBN = 128, GBK = 16, GPAD = 16;

enum { GEPI_STORE = 0, GEPI_BIAS_SIGMOID = 1, GEPI_RELU_MASK = 2 };

template <bool A_KC, bool B_NC, int EPI>
__global__ __launch_bounds__(kBlk) void gan_gemm_kernel(int M, int N, int K, const float *__restrict__ A, long long sam, long long sak,
                                                       const float *__restrict__ B, long long sbk, long long sbn, float *__restrict__ C, long long ldc,
                                                       const float *__restrict__ bias, const float *__restrict__ aux) {
    __shared__ float As[GBK][GBM + GPAD];
    __shared__ float Bs[GBK][GBN + GPAD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const long long m0 = (long long)blockIdx.y * GBM, n0 = (long long)blockIdx.x * GBN;
    f32x4v acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4v){0.f, 0.f, 0.f, 0.f};
    // the next K slice is loaded into registers while the matrix cores work on the current one (staged in LDS)
    constexpr int NA = GBM * GBK / kBlk, NB = GBN * GBK / kBlk;
    float ra[NA], rb[NB];
    auto load = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + kBlk * i;
            const int kk = A_KC ? (e % GBK) : (e / GBM), mm = A_KC ? (e / GBK) : (e % GBM);
            const long long m = m0 + mm, k = k0 + kk;
            ra[i] = (m < M && k < K) ? A[m * sam + k * sak] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + kBlk * i;
            const int kk = B_NC ? (e / GBN) : (e % GBK), nn = B_NC ? (e % GBN) : (e / GBK);
            const long long n = n0 + nn, k = k0 + kk;
            rb[i] = (n < N && k < K) ? B[k * sbk + n * sbn] : 0.f;
        }
    };
    load(0);
    for (int k0 = 0; k0 < K; k0 += GBK) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int e = tid + kBlk * i;
            As[A_KC ? (e % GBK) : (e / GBM)][A_KC ? (e / GBK) : (e % GBM)] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int e = tid + kBlk * i;
            Bs[B_NC ? (e / GBN) : (e % GBK)][B_NC ? (e % GBN) : (e / GBK)] = rb[i];
        }
        __syncthreads();
        if (k0 + GBK < K) load(k0 + GBK);
#pragma unroll
        for (int ks = 0; ks < GBK; ks += 4) {
            float av[4], bv[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) { av[t] = As[ks + q][wm + 16 * t + c]; bv[t] = Bs[ks + q][wn + 16 * t + c]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // acc[i][j][r] = C[m0 + wm + 16 i + 4 q + r][n0 + wn + 16 j + c]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long long n = n0 + wn + 16 * j + c;
        if (n >= N) continue;
        const float b = EPI == GEPI_BIAS_SIGMOID ? bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long m = m0 + wm + 16 * i + 4 * q + r;
                if (m >= M) continue;
                float v = acc[i][j][r];
                if (EPI == GEPI_BIAS_SIGMOID) v = 1.f / (1.f + expf(-(v + b)));
                if (EPI == GEPI_RELU_MASK) v = aux[m * ldc + n] > 0.f ? v : 0.f;
                C[m * ldc + n] = v;
            }
    }
}

// ------------------------------------------------------------------------------------------------ sparse rows x dense
// out[r, n] = (bias ? bias[n] : 0) + sum_{k in row r} val[k] X[col[k], n], then relu if asked.  Grid (n_rows, ceil(N / 256)): one workgroup per
// row and 256-column strip, so a long row (a popular item's column of the template, for dW1) is spread over N / 256 workgroups.  Entries are
// summed in CSR order, four gathers in flight per lane.
__global__ __launch_bounds__(kBlk) void gan_spmm_kernel(int n_rows, int N, const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                       const float *__restrict__ val, const float *__restrict__ X, const float *__restrict__ bias,
                                                       int relu, float *__restrict__ out) {
    const long long r = blockIdx.x;
    const int n = blockIdx.y * kBlk + threadIdx.x;
    if (n >= N) return;
    const long long b = rowptr[r], e = rowptr[r + 1];
    float a = 0.f;
    long long k = b;
    for (; k + 4 <= e; k += 4) {
        const float x0 = X[(long long)col[k] * N + n], x1 = X[(long long)col[k + 1] * N + n];
        const float x2 = X[(long long)col[k + 2] * N + n], x3 = X[(long long)col[k + 3] * N + n];
        a = fmaf(val[k], x0, a); a = fmaf(val[k + 1], x1, a); a = fmaf(val[k + 2], x2, a); a = fmaf(val[k + 3], x3, a);
    }
    for (; k < e; ++k) a = fmaf(val[k], X[(long long)col[k] * N + n], a);
    if (bias) a += bias[n];
    if (relu) a = a > 0.f ? a : 0.f;
    out[r * N + n] = a;
}

// 32 x 32 LDS tile transpose: At[c][r] = A[r][c], A [R, Cn]
__global__ __launch_bounds__(kBlk) void gan_transpose_kernel(const float *__restrict__ A, int R, int Cn, float *__restrict__ At) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const long long r0 = (long long)blockIdx.y * 32, c0 = (long long)blockIdx.x * 32;
    for (int y = ty; y < 32; y += 8) {
        const long long r = r0 + y, cc = c0 + tx;
        if (r < R && cc < Cn) t[y][tx] = A[r * Cn + cc];
    }
    __syncthreads();
    for (int y = ty; y < 32; y += 8) {
        const long long cc = c0 + y, r = r0 + tx;
        if (r < R && cc < Cn) At[cc * R + r] = t[tx][y];
    }
}

// ------------------------------------------------------------------------------------------------ fixed-order block reduction
__device__ __forceinline__ float block_sum(float v, float *sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    const float out = sh[0];
    __syncthreads();
    return out;
}

// per row r of Y [F, S] (dense template Td [F, S]): rows[r] = (Y_r . w_D, Td_r . w_D, sum_c (Y - Td)^2, sum_{c >= S - T} (1 - Y))
__global__ __launch_bounds__(kBlk) void gan_rows_kernel(const float *__restrict__ Y, const float *__restrict__ Td, int S, int T,
                                                       const float *__restrict__ wD, float *__restrict__ rows) {
    __shared__ float sh[kBlk];
    const long long r = blockIdx.x;
    const float *y = Y + r * S, *t = Td + r * S;
    float yw = 0.f, tw = 0.f, sq = 0.f, sh_s = 0.f;
    for (int c = threadIdx.x; c < S; c += kBlk) {
        const float yv = y[c], tv = t[c], w = wD[c], d = yv - tv;
        yw = fmaf(yv, w, yw);
        tw = fmaf(tv, w, tw);
        sq = fmaf(d, d, sq);
        if (c >= S - T) sh_s += 1.f - yv;
    }
    yw = block_sum(yw, sh); tw = block_sum(tw, sh); sq = block_sum(sq, sh); sh_s = block_sum(sh_s, sh);
    if (threadIdx.x == 0) { rows[4 * r] = yw; rows[4 * r + 1] = tw; rows[4 * r + 2] = sq; rows[4 * r + 3] = sh_s; }
}

// one workgroup: losses and the D step's per-row coefficients from rows [F, 4] and b_D.
// out: [0] loss1 (D step), [1] loss2 (G step), [2] dL1/db_D;  coef [2 F]: a_r = -(1 - D(T_r)) / F, b_r = D(Y_r) / F (dL1/dlogits);
// pf [F] = D(Y_r)
__global__ __launch_bounds__(kBlk) void gan_loss_kernel(const float *__restrict__ rows, int F, int S, const float *__restrict__ bD,
                                                       float *__restrict__ out, float *__restrict__ coef, float *__restrict__ pf) {
    __shared__ float sh[kBlk];
    const float b = bD[0], invF = 1.f / (float)F;
    float lr = 0.f, lf = 0.f, ls = 0.f, lq = 0.f, db = 0.f;
    for (int r = threadIdx.x; r < F; r += kBlk) {
        const float pr = 1.f / (1.f + expf(-(rows[4 * r + 1] + b))), p = 1.f / (1.f + expf(-(rows[4 * r] + b)));
        lr += logf(pr);
        lf += logf(1.f - p);
        ls += rows[4 * r + 3] * rows[4 * r + 3];
        lq += rows[4 * r + 2];
        const float a = -(1.f - pr) * invF, bb = p * invF;
        db += a + bb;
        coef[r] = a;
        coef[F + r] = bb;
        pf[r] = p;
    }
    lr = block_sum(lr, sh); lf = block_sum(lf, sh); ls = block_sum(ls, sh); lq = block_sum(lq, sh); db = block_sum(db, sh);
    if (threadIdx.x == 0) {
        const float m = lr * invF + lf * invF;
        out[0] = -m;
        out[1] = m + ls * invF + lq / ((float)F * (float)S);
        out[2] = db;
    }
}

// dZ2 = dL2/dY * Y (1 - Y),  dL2/dY = 2 (Y - Td) / (F S) - (2 s_r / F) [c >= S - T] - (D(Y_r) / F) w_D[c]
__global__ __launch_bounds__(kBlk) void gan_dz2_kernel(const float *__restrict__ Y, const float *__restrict__ Td, const float *__restrict__ rows,
                                                      const float *__restrict__ pf, const float *__restrict__ wD, int F, int S, int T,
                                                      float *__restrict__ dZ2) {
    const long long r = blockIdx.x;
    const float invF = 1.f / (float)F, c1 = 2.f / ((float)F * (float)S), sr = 2.f * rows[4 * r + 3] * invF, p = pf[r] * invF;
    for (int c = threadIdx.x; c < S; c += kBlk) {
        const float y = Y[r * S + c];
        float g = c1 * (y - Td[r * S + c]) - p * wD[c];
        if (c >= S - T) g -= sr;
        dZ2[r * S + c] = g * (y * (1.f - y));
    }
}

// column sums in fixed order: part[chunk][c] = sum_{r in chunk} (wa ? wa[r] : 1) A[r, c] + (Bm ? wb[r] Bm[r, c] : 0)
__global__ __launch_bounds__(kBlk) void gan_colsum_kernel(const float *__restrict__ A, const float *__restrict__ wa, const float *__restrict__ Bm,
                                                         const float *__restrict__ wb, int F, int S, int chunk, float *__restrict__ part) {
    const long long c = (long long)blockIdx.x * kBlk + threadIdx.x;
    if (c >= S) return;
    const long long r0 = (long long)blockIdx.y * chunk, r1 = r0 + chunk < F ? r0 + chunk : F;
    float s = 0.f;
    for (long long r = r0; r < r1; ++r) {
        s = fmaf(wa ? wa[r] : 1.f, A[r * S + c], s);
        if (Bm) s = fmaf(wb[r], Bm[r * S + c], s);
    }
    part[(long long)blockIdx.y * S + c] = s;
}

__global__ __launch_bounds__(kBlk) void gan_fold_kernel(const float *__restrict__ part, int n_part, int S, float *__restrict__ out) {
    const long long c = (long long)blockIdx.x * kBlk + threadIdx.x;
    if (c >= S) return;
    float s = 0.f;
    for (int p = 0; p < n_part; ++p) s += part[(long long)p * S + c];
    out[c] = s;
}

// ------------------------------------------------------------------------------------------------ template
// Counter hash of (seed, call, row, item) -> uniform in [0, 1) with 24 bits (splitmix64 finaliser).
__device__ __forceinline__ bool hash_keep(uint64_t key, long long r, long long item, float p) {
    const uint64_t u = arl_splitmix64(key ^ ((uint64_t)r * 0x100000000ull + (uint64_t)item)) >> 40;
    return (float)u * (1.f / 16777216.f) < p;
}

__device__ __forceinline__ float csr_lookup(const int64_t *__restrict__ rowptr, const int32_t *__restrict__ col, const float *__restrict__ val,
                                            long long r, int j) {
    long long lo = rowptr[r], hi = rowptr[r + 1];
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (col[mid] < j) lo = mid + 1; else hi = mid;
    }
    return (lo < rowptr[r + 1] && col[lo] == j) ? val[lo] : 0.f;
}

struct GanTemplateArgs {
    int F, S, n_users;
    const int32_t *user_set;                               // [F]
    const int64_t *rowptr; const int32_t *col; const float *val;   // U x I interaction CSR, ascending columns per row
    const int32_t *pos;                                    // [I]: position in selectItem or -1
    const int32_t *items;                                  // [S]: selectItem
    const uint8_t *mask;                                   // [F, S] injected mask, or NULL: counter hash
    const float *item_p;                                   // [I] Bernoulli probabilities (hash source)
    uint64_t key;
    const int64_t *out_ptr;                                // fill pass: [F + 1] row offsets; count pass: NULL
    int64_t *counts;                                       // count pass: [F]
    int32_t *out_col; float *out_val;
};

// one wave per template row r: entries of interaction row user_set[r] whose item c is selected give column j = pos[c] and value
// interact[r, j] * mask[r, j] (the reference's local-row / position quirk), kept in the interaction row's order; explicit zeros stay.
__global__ __launch_bounds__(kBlk) void gan_template_kernel(GanTemplateArgs a) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
    if (r >= a.F) return;
    const long long u = a.user_set[r];
    const long long b = a.rowptr[u], e = a.rowptr[u + 1];
    long long w = a.out_ptr ? a.out_ptr[r] : 0;
    for (long long k0 = b; k0 < e; k0 += 64) {
        const long long k = k0 + lane;
        const int j = k < e ? a.pos[a.col[k]] : -1;
        const unsigned long long bal = __ballot(j >= 0);
        if (a.out_ptr && j >= 0) {
            const long long slot = w + __popcll(bal & ((1ull << lane) - 1ull));
            float m;
            if (a.mask) m = (float)a.mask[r * a.S + j];
            else m = hash_keep(a.key, r, a.items[j], a.item_p[a.items[j]]) ? 1.f : 0.f;
            a.out_col[slot] = j;
            a.out_val[slot] = csr_lookup(a.rowptr, a.col, a.val, r, j) * m;
        }
        w += __popcll(bal);
    }
    if (!a.out_ptr && lane == 0) a.counts[r] = w;
}

__global__ __launch_bounds__(kBlk) void gan_hash_mask_kernel(int F, int S, const int32_t *__restrict__ items, const float *__restrict__ item_p,
                                                            uint64_t key, uint8_t *__restrict__ out) {
    const long long t = (long long)blockIdx.x * kBlk + threadIdx.x;
    if (t >= (long long)F * S) return;
    const long long r = t / S, j = t - r * S;
    out[t] = hash_keep(key, r, items[j], item_p[items[j]]) ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------ threshold / compact
// one wave per row: count pass (out_ptr NULL) writes counts[r] = #{c : Y[r, c] > thr}; fill pass writes the columns in ascending order
__global__ __launch_bounds__(kBlk) void gan_threshold_kernel(const float *__restrict__ Y, int F, int S, float thr, const int64_t *__restrict__ out_ptr,
                                                            int64_t *__restrict__ counts, int32_t *__restrict__ out_col) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
    if (r >= F) return;
    long long w = out_ptr ? out_ptr[r] : 0;
    for (int c0 = 0; c0 < S; c0 += 64) {
        const int c = c0 + lane;
        const bool keep = c < S && Y[r * S + c] > thr;
        const unsigned long long bal = __ballot(keep);
        if (out_ptr && keep) out_col[w + __popcll(bal & ((1ull << lane) - 1ull))] = c;
        w += __popcll(bal);
    }
    if (!out_ptr && lane == 0) counts[r] = w;
}

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

template <int EPI>
int launch_gemm(int M, int N, int K, const float *A, long long sam, long long sak, const float *B, long long sbk, long long sbn, float *C,
                const float *bias, const float *aux, hipStream_t st) {
    const dim3 grid(cdiv(N, GBN), cdiv(M, GBM));
    const bool akc = sak == 1, bnc = sbn == 1;
#define GAN_GEMM_LAUNCH(AK, BN)                                                                                                           \
    hipLaunchKernelGGL((gan_gemm_kernel<AK, BN, EPI>), grid, dim3(kBlk), 0, st, M, N, K, A, sam, sak, B, sbk, sbn, C, (long long)N, bias, aux)
    if (akc && bnc) GAN_GEMM_LAUNCH(true, true);
    else if (akc) GAN_GEMM_LAUNCH(true, false);
    else if (bnc) GAN_GEMM_LAUNCH(false, true);
    else GAN_GEMM_LAUNCH(false, false);
#undef GAN_GEMM_LAUNCH
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

constexpr long long kGanMaxElems = 0x7fffffffLL;          // every F x S and S x S operand is indexed within this by the row kernels

}  // namespace

extern "C" {

int arl_gan_gemm_f32(int64_t M, int64_t N, int64_t K, const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C,
                     int32_t epilogue, const float *bias, const float *aux, arl_stream_t stream) {
    if (!A || !B || !C) return ARL_E_NULL;
    if (M < 0 || N < 0 || K < 0 || epilogue < 0 || epilogue > 2) return ARL_E_ARG;
    if ((sak != 1 && sam != 1) || (sbn != 1 && sbk != 1)) return ARL_E_ARG;
    if ((epilogue == GEPI_BIAS_SIGMOID && !bias) || (epilogue == GEPI_RELU_MASK && !aux)) return ARL_E_NULL;
    if (M * N > kGanMaxElems || M * K > kGanMaxElems || K * N > kGanMaxElems || M > 0x7fff0000LL || N > 0x7fff0000LL) return ARL_E_RANGE;
    if (M == 0 || N == 0) return ARL_OK;
    hipStream_t st = (hipStream_t)stream;
    if (epilogue == GEPI_STORE) return launch_gemm<GEPI_STORE>((int)M, (int)N, (int)K, A, sam, sak, B, sbk, sbn, C, bias, aux, st);
    if (epilogue == GEPI_BIAS_SIGMOID) return launch_gemm<GEPI_BIAS_SIGMOID>((int)M, (int)N, (int)K, A, sam, sak, B, sbk, sbn, C, bias, aux, st);
    return launch_gemm<GEPI_RELU_MASK>((int)M, (int)N, (int)K, A, sam, sak, B, sbk, sbn, C, bias, aux, st);
}

int arl_gan_spmm_f32(int64_t n_rows, int64_t N, const int64_t *rowptr, const int32_t *col, const float *val, const float *X, const float *bias,
                     int32_t relu, float *out, arl_stream_t stream) {
    if (!rowptr || !out || (!X && N > 0)) return ARL_E_NULL;
    if (n_rows < 0 || N < 0) return ARL_E_ARG;
    if (n_rows * N > kGanMaxElems || n_rows > 0x7fffffffLL) return ARL_E_RANGE;
    if (n_rows == 0 || N == 0) return ARL_OK;
    hipLaunchKernelGGL(gan_spmm_kernel, dim3((unsigned)n_rows, cdiv(N, kBlk)), dim3(kBlk), 0, (hipStream_t)stream, (int)n_rows, (int)N, rowptr, col, val, X, bias,
                       (int)relu, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gan_transpose_f32(const float *A, int64_t R, int64_t Cn, float *At, arl_stream_t stream) {
    if (!A || !At) return ARL_E_NULL;
    if (R < 0 || Cn < 0 || A == At) return ARL_E_ARG;
    if (R * Cn > kGanMaxElems) return ARL_E_RANGE;
    if (R == 0 || Cn == 0) return ARL_OK;
    hipLaunchKernelGGL(gan_transpose_kernel, dim3(cdiv(Cn, 32), cdiv(R, 32)), dim3(kBlk), 0, (hipStream_t)stream, A, (int)R, (int)Cn, At);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gan_rows_f32(const float *Y, const float *Td, int64_t F, int64_t S, int64_t T, const float *wD, const float *bD, float *rows, float *losses,
                     float *coef, float *pf, arl_stream_t stream) {
    if (!Y || !Td || !wD || !bD || !rows || !losses || !coef || !pf) return ARL_E_NULL;
    if (F < 1 || S < 1 || T < 0 || T > S) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gan_rows_kernel, dim3((unsigned)F), dim3(kBlk), 0, st, Y, Td, (int)S, (int)T, wD, rows);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(gan_loss_kernel, dim3(1), dim3(kBlk), 0, st, rows, (int)F, (int)S, bD, losses, coef, pf);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gan_dz2_f32(const float *Y, const float *Td, const float *rows, const float *pf, const float *wD, int64_t F, int64_t S, int64_t T, float *dZ2,
                    arl_stream_t stream) {
    if (!Y || !Td || !rows || !pf || !wD || !dZ2) return ARL_E_NULL;
    if (F < 1 || S < 1 || T < 0 || T > S) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    hipLaunchKernelGGL(gan_dz2_kernel, dim3((unsigned)F), dim3(kBlk), 0, (hipStream_t)stream, Y, Td, rows, pf, wD, (int)F, (int)S, (int)T, dZ2);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_gan_colsum_workspace_bytes(int64_t F, int64_t S) {
    if (F < 1 || S < 1) return 0;
    const int64_t chunk = 64, n_part = (F + chunk - 1) / chunk;
    return n_part * S * (int64_t)sizeof(float);
}

int arl_gan_colsum_f32(const float *A, const float *wa, const float *Bm, const float *wb, int64_t F, int64_t S, float *out, void *workspace,
                       arl_stream_t stream) {
    if (!A || !out || !workspace || (Bm && !wb)) return ARL_E_NULL;
    if (F < 1 || S < 1) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    const int chunk = 64;
    const int n_part = (int)((F + chunk - 1) / chunk);
    hipStream_t st = (hipStream_t)stream;
    float *part = (float *)workspace;
    hipLaunchKernelGGL(gan_colsum_kernel, dim3(cdiv(S, kBlk), (unsigned)n_part), dim3(kBlk), 0, st, A, wa, Bm, wb, (int)F, (int)S, chunk, part);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(gan_fold_kernel, dim3(cdiv(S, kBlk)), dim3(kBlk), 0, st, part, n_part, (int)S, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

// the key of a call: one hash of (seed, call), shared by every kernel of the library that draws from the counter hash
uint64_t arl_gan_hash_key(uint64_t seed, uint64_t call) { return arl_splitmix64(seed ^ (call * 0x9E3779B97F4A7C15ull)); }

int arl_gan_template_i32(int64_t F, int64_t S, int64_t n_users, const int32_t *user_set, const int64_t *rowptr, const int32_t *col, const float *val,
                         const int32_t *pos, const int32_t *items, const uint8_t *mask, const float *item_p, uint64_t seed, uint64_t call,
                         const int64_t *out_ptr, int64_t *counts, int32_t *out_col, float *out_val, arl_stream_t stream) {
    if (!user_set || !rowptr || !col || !val || !pos || !items) return ARL_E_NULL;
    if (!mask && !item_p) return ARL_E_NULL;
    if (out_ptr ? (!out_col || !out_val) : !counts) return ARL_E_NULL;
    if (F < 0 || S < 1 || n_users < F) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    if (F == 0) return ARL_OK;
    GanTemplateArgs a{(int)F, (int)S, (int)n_users, user_set, rowptr, col, val, pos, items, mask, item_p, arl_gan_hash_key(seed, call), out_ptr, counts,
                      out_col, out_val};
    hipLaunchKernelGGL(gan_template_kernel, dim3(cdiv(F, kBlk / 64)), dim3(kBlk), 0, (hipStream_t)stream, a);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gan_hash_mask_u8(int64_t F, int64_t S, const int32_t *items, const float *item_p, uint64_t seed, uint64_t call, uint8_t *out,
                         arl_stream_t stream) {
    if (!items || !item_p || !out) return ARL_E_NULL;
    if (F < 0 || S < 1) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    if (F == 0) return ARL_OK;
    hipLaunchKernelGGL(gan_hash_mask_kernel, dim3(cdiv(F * S, kBlk)), dim3(kBlk), 0, (hipStream_t)stream, (int)F, (int)S, items, item_p,
                       arl_gan_hash_key(seed, call), out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gan_threshold_f32(const float *Y, int64_t F, int64_t S, float thr, const int64_t *out_ptr, int64_t *counts, int32_t *out_col,
                          arl_stream_t stream) {
    if (!Y || (out_ptr ? !out_col : !counts)) return ARL_E_NULL;
    if (F < 0 || S < 1) return ARL_E_ARG;
    if (F * S > kGanMaxElems) return ARL_E_RANGE;
    if (F == 0) return ARL_OK;
    hipLaunchKernelGGL(gan_threshold_kernel, dim3(cdiv(F, kBlk / 64)), dim3(kBlk), 0, (hipStream_t)stream, Y, (int)F, (int)S, thr, out_ptr, counts,
                       out_col);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

// arl_profilegen.hip -- GSPAttack's profile generator on gfx950 (reference attack/Black/GSPAttack.py:120-130, 201-202, 224-231, as repaired in
// arlib_amd/attack/Black/GSPAttack.py): the pair-MLP head over every (fake user, item) pair and the relaxed Gumbel top-k over its logits.
//
// a. Pair-MLP head.  A [F, H] = E_f W1[:, :d]^T + b1, B [I, H] = E_i W1[:, d:]^T (two GEMMs the caller keeps in torch), w2 [H], b2 [1]:
//        x[f, i] = b2 + sum_h w2[h] relu(A[f, h] + B[i, h])
//    and for an upstream g [F, I], with the ReLU derivative 0 at exactly 0:
//        dA[f, h] = w2[h] sum_i g[f, i] [A[f, h] + B[i, h] > 0],      dB[i, h] = w2[h] sum_f g[f, i] [A[f, h] + B[i, h] > 0],
//        dw2[h] = sum_{f, i} g[f, i] relu(A[f, h] + B[i, h]),         db2 = sum g.
//    No F x I x H tensor exists: pmlp_fwd_kernel keeps 8 fake users x 256 items per workgroup and streams H through LDS 32 columns at a time;
//    pmlp_bwd_rows_kernel (lanes on h, 8 fake users in registers, items streamed in splits) gives dA and dw2's per-row terms, pmlp_bwd_cols_kernel
//    (lanes on h, 8 items per wave in registers, fake users streamed) gives dB.
//
// b. Relaxed Gumbel top-k (gumbel_topk_relaxed's semantics).  Round r, over the items not picked before: z = (x + g_r) / tau, y_r = softmax(z),
//    j_r = argmax z (lowest index on a tie); S = sum_r y_r.  gtk_rounds_kernel: one workgroup per fake user, the rounds in sequence, one pass per
//    round with a running (max, sum, argmax); it leaves picks [F, k], the per-round (max, sum) and log-sum-exp.  gtk_accum_kernel: one thread per
//    (f, i) walks the rounds with the saved statistics: S (forward), c_r = sum_j y_r[j] dS[j] (per-tile partials) and
//    dx[f, i] = (1 / tau) sum_r y_r[i] (dS[i] - c_r).  y_r = exp(z - max_r) / sum_r, as torch.softmax forms it.
//    Noise: the caller's [k, F, I] tensor, or g = -log(-log u) from a counter hash of (seed, call, r, f, i) (splitmix64, 24 bits, u in (0, 1)).
//
// Rules kept throughout: no atomics and fixed-order reductions (bit-identical from run to run); long sums run in fp32 per
// tile (16 to 64 terms) and in double across tiles; contraction is off wherever two kernels must form the same value.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_util.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr int kMaxH = 1024;                      // PAIR_MLP_MAX_H
constexpr int kMaxK = 512;                       // GUMBEL_MAX_K
constexpr int64_t kMaxF = 8 * 65535;             // fake users: 8 per workgroup on gridDim.y
constexpr int64_t kMaxI = 0x7fffffffll - 2048;   // items: every i0 + tid of the kernels' int arithmetic stays in int32
constexpr int TF = 8;                            // fake users per workgroup (forward, rows backward)
constexpr int HC = 32;                           // hidden columns per LDS stage of the forward
constexpr int IS = 64;                           // items per stage of the rows backward
constexpr int TI = 8, FS = 64;                   // items per wave and fake users per stage of the columns backward
constexpr int kRoundsBlk = 1024;                 // threads of the one workgroup a fake user's rounds run in
constexpr int kSumBlocks = 1024;                 // partial sums of db2

// ================================================================================================ pair-MLP head
__global__ __launch_bounds__(kBlk) void pmlp_fwd_kernel(const float *__restrict__ A, const float *__restrict__ B, const float *__restrict__ w2,
                                                         const float *__restrict__ b2, int F, int I, int H, float *__restrict__ x) {
    __shared__ float tile[kBlk * (HC + 1)];      // [item][h], rows padded to 33 words: a wave's 64 rows fall on distinct banks
    const int tid = threadIdx.x;
    const int i0 = blockIdx.x * kBlk, f0 = blockIdx.y * TF, i = i0 + tid;
    double acc[TF];
#pragma unroll
    for (int j = 0; j < TF; ++j) acc[j] = 0.0;
    for (int h0 = 0; h0 < H; h0 += HC) {
        const int hc = min(HC, H - h0);
        __syncthreads();
#pragma unroll
        for (int n = 0; n < HC; ++n) {
            const int e = tid + n * kBlk, row = e / HC, col = e % HC, ii = i0 + row;
            tile[row * (HC + 1) + col] = (ii < I && col < hc) ? B[(size_t)ii * H + h0 + col] : 0.f;
        }
        __syncthreads();
        float c[TF];
#pragma unroll
        for (int j = 0; j < TF; ++j) c[j] = 0.f;
        for (int hh = 0; hh < hc; ++hh) {
            const float b = tile[tid * (HC + 1) + hh], w = w2[h0 + hh];
#pragma unroll
            for (int j = 0; j < TF; ++j) {
                const float a = A[(size_t)min(f0 + j, F - 1) * H + h0 + hh];        // wave-uniform: a scalar load
                c[j] = fmaf(w, fmaxf(a + b, 0.f), c[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < TF; ++j) acc[j] += (double)c[j];                       // 32 terms in fp32, the stages in double
    }
    if (i >= I) return;
    const double bias = (double)b2[0];
#pragma unroll
    for (int j = 0; j < TF; ++j)
        if (f0 + j < F) x[(size_t)(f0 + j) * I + i] = (float)(acc[j] + bias);
}

// partM[split][f][h] = sum over the split's items of g[f, i] [A[f, h] + B[i, h] > 0],   partP[split][f][h] = the same with relu(.) for [. > 0]
__global__ __launch_bounds__(kBlk) void pmlp_bwd_rows_kernel(const float *__restrict__ g, const float *__restrict__ A, const float *__restrict__ B, int F,
                                                              int I, int H, int split_len, double *__restrict__ partM, double *__restrict__ partP) {
    __shared__ __align__(16) float gs[2][IS * TF];             // [item][fake user]
    __shared__ double red[kWaves - 1][2 * TF][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h = blockIdx.x * 64 + lane, hh = min(h, H - 1), f0 = blockIdx.y * TF;
    const int i_begin = blockIdx.z * split_len, i_end = min(I, i_begin + split_len);
    float a[TF];
#pragma unroll
    for (int j = 0; j < TF; ++j) a[j] = A[(size_t)min(f0 + j, F - 1) * H + hh];
    double M[TF], P[TF];
#pragma unroll
    for (int j = 0; j < TF; ++j) M[j] = P[j] = 0.0;
    const int nst = (i_end - i_begin + IS - 1) / IS;
    // a stage is 8 rows of 64 upstream values, two per thread; items past the split's end and fake users past F read as 0
#define PMLP_ROWS_LOAD(ST, BUF)                                                                                 \
    do {                                                                                                        \
        _Pragma("unroll") for (int n = 0; n < 2; ++n) {                                                         \
            const int e = tid + n * kBlk, j = e / IS, ii = e % IS, it = i_begin + (ST) * IS + ii;               \
            gs[BUF][ii * TF + j] = (f0 + j < F && it < i_end) ? g[(size_t)(f0 + j) * I + it] : 0.f;             \
        }                                                                                                       \
    } while (0)
    if (nst > 0) PMLP_ROWS_LOAD(0, 0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) PMLP_ROWS_LOAD(st + 1, buf ^ 1);
        float m[TF], p[TF];
#pragma unroll
        for (int j = 0; j < TF; ++j) m[j] = p[j] = 0.f;
#pragma unroll 4
        for (int q = 0; q < IS / kWaves; ++q) {
            const int ii = q * kWaves + wv, it = min(i_begin + st * IS + ii, I - 1);
            const float b = B[(size_t)it * H + hh];
            const float4 g0 = *reinterpret_cast<const float4 *>(&gs[buf][ii * TF]), g1 = *reinterpret_cast<const float4 *>(&gs[buf][ii * TF + 4]);
            const float gj[TF] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int j = 0; j < TF; ++j) {
                const float t = a[j] + b;
                m[j] += t > 0.f ? gj[j] : 0.f;
                p[j] = fmaf(gj[j], fmaxf(t, 0.f), p[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < TF; ++j) { M[j] += (double)m[j]; P[j] += (double)p[j]; }      // 16 terms in fp32, the stages in double
        __syncthreads();
    }
#undef PMLP_ROWS_LOAD
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < TF; ++j) { red[wv - 1][j][lane] = M[j]; red[wv - 1][TF + j][lane] = P[j]; }
    }
    __syncthreads();
    if (wv != 0 || h >= H) return;
#pragma unroll
    for (int j = 0; j < TF; ++j) {
        if (f0 + j >= F) continue;
        double sm = M[j], sp = P[j];
#pragma unroll
        for (int w = 0; w < kWaves - 1; ++w) { sm += red[w][j][lane]; sp += red[w][TF + j][lane]; }
        const size_t o = ((size_t)blockIdx.z * F + (f0 + j)) * H + h;
        partM[o] = sm;
        partP[o] = sp;
    }
}

// dB[i, h] = w2[h] sum_f g[f, i] [A[f, h] + B[i, h] > 0]: a wave holds 8 items, the fake users pass through LDS 64 at a time
__global__ __launch_bounds__(kBlk) void pmlp_bwd_cols_kernel(const float *__restrict__ g, const float *__restrict__ A, const float *__restrict__ B,
                                                              const float *__restrict__ w2, int F, int I, int H, float *__restrict__ dB) {
    constexpr int NI = kWaves * TI;              // 32 items per workgroup
    __shared__ __align__(16) float gs[2][FS * NI];             // [fake user][item]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int h = blockIdx.y * 64 + lane, hh = min(h, H - 1), i0 = blockIdx.x * NI;
    float b[TI];
#pragma unroll
    for (int j = 0; j < TI; ++j) b[j] = B[(size_t)min(i0 + wv * TI + j, I - 1) * H + hh];
    double D[TI];
#pragma unroll
    for (int j = 0; j < TI; ++j) D[j] = 0.0;
    const int nst = (F + FS - 1) / FS;
#define PMLP_COLS_LOAD(ST, BUF)                                                                                 \
    do {                                                                                                        \
        _Pragma("unroll") for (int n = 0; n < FS * NI / kBlk; ++n) {                                            \
            const int e = tid + n * kBlk, ff = e / NI, ii = e % NI, f = (ST) * FS + ff;                         \
            gs[BUF][e] = (f < F && i0 + ii < I) ? g[(size_t)f * I + i0 + ii] : 0.f;                             \
        }                                                                                                       \
    } while (0)
    PMLP_COLS_LOAD(0, 0);
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) PMLP_COLS_LOAD(st + 1, buf ^ 1);
        float d[TI];
#pragma unroll
        for (int j = 0; j < TI; ++j) d[j] = 0.f;
#pragma unroll 4
        for (int ff = 0; ff < FS; ++ff) {
            const float a = A[(size_t)min(st * FS + ff, F - 1) * H + hh];         // rows past F carry g = 0
            const float4 g0 = *reinterpret_cast<const float4 *>(&gs[buf][ff * NI + wv * TI]), g1 = *reinterpret_cast<const float4 *>(&gs[buf][ff * NI + wv * TI + 4]);
            const float gj[TI] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
            for (int j = 0; j < TI; ++j) d[j] += a + b[j] > 0.f ? gj[j] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < TI; ++j) D[j] += (double)d[j];                        // 64 terms in fp32, the stages in double
        __syncthreads();
    }
#undef PMLP_COLS_LOAD
    if (h >= H) return;
    const float w = w2[h];
#pragma unroll
    for (int j = 0; j < TI; ++j) {
        const int i = i0 + wv * TI + j;
        if (i < I) dB[(size_t)i * H + h] = w * (float)D[j];
    }
}

// part[b] = the sum of workgroup b's strided share of g, in double
__global__ __launch_bounds__(kBlk) void pmlp_sum_kernel(const float *__restrict__ g, size_t n, double *__restrict__ part) {
    __shared__ double red[kBlk];
    double v = 0.0;
    for (size_t e = (size_t)blockIdx.x * kBlk + threadIdx.x; e < n; e += (size_t)gridDim.x * kBlk) v += (double)g[e];
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kBlk / 2; s > 0; s >>= 1) { if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(kBlk) void pmlp_dA_kernel(const double *__restrict__ partM, const float *__restrict__ w2, int F, int H, int ns, float *__restrict__ dA) {
    const size_t n = (size_t)F * H, e = (size_t)blockIdx.x * kBlk + threadIdx.x;
    if (e >= n) return;
    double s = partM[e];
    for (int k = 1; k < ns; ++k) s += partM[(size_t)k * n + e];                   // the splits in ascending order
    dA[e] = w2[e % H] * (float)s;
}

// dw2[h] = sum_f sum_split partP[split][f][h] (a wave takes every fourth fake user, the waves are folded in order); workgroup 0 also folds db2
__global__ __launch_bounds__(kBlk) void pmlp_finish_kernel(const double *__restrict__ partP, int F, int H, int ns, const double *__restrict__ sum_part, int n_sum,
                                                            float *__restrict__ dw2, float *__restrict__ db2) {
    __shared__ double red[kBlk];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, h = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (h < H)
        for (int f = wv; f < F; f += kWaves)
            for (int k = 0; k < ns; ++k) s += partP[((size_t)k * F + f) * H + h];
    red[tid] = s;
    __syncthreads();
    if (wv == 0 && h < H) dw2[h] = (float)(((red[lane] + red[64 + lane]) + red[128 + lane]) + red[192 + lane]);
    if (blockIdx.x != 0) return;
    __syncthreads();
    double v = 0.0;
    for (int e = tid; e < n_sum; e += kBlk) v += sum_part[e];
    red[tid] = v;
    __syncthreads();
    for (int st = kBlk / 2; st > 0; st >>= 1) { if (tid < st) red[tid] += red[tid + st]; __syncthreads(); }
    if (tid == 0) db2[0] = (float)red[0];
}

// splits of the items in the rows backward: about 1 024 workgroups, at least 256 items per split
int pmlp_splits(int64_t F, int64_t I, int64_t H) {
    const int64_t base = ((H + 63) / 64) * ((F + TF - 1) / TF);
    int64_t s = (1024 + base - 1) / base;
    const int64_t max_s = (I + 255) / 256;
    if (s > max_s) s = max_s;
    return (int)(s < 1 ? 1 : s);
}

int pmlp_sum_blocks(int64_t n) {
    const int64_t b = (n + 16 * kBlk - 1) / (16 * kBlk);
    return (int)(b > kSumBlocks ? kSumBlocks : b);
}

int pmlp_shape(int64_t F, int64_t I, int64_t H) {
    if (H > kMaxH) return ARL_E_DIM;
    if (F <= 0 || I <= 0 || H <= 0) return ARL_E_ARG;
    if (F > kMaxF || I > kMaxI) return ARL_E_RANGE;
    return ARL_OK;
}

// ================================================================================================ relaxed Gumbel top-k
__device__ __forceinline__ uint64_t pg_rowkey(uint64_t key, int r, int f) { return arl_splitmix64(key ^ (((uint64_t)(uint32_t)r << 32) | (uint64_t)(uint32_t)f)); }

// g = -log(-log u), u = (n + 1/2) 2^-24 for the 24-bit draw n: u lies in the open interval, so g is finite ([-2.85, 17.4]).  n + 1/2 is exact
// in fp32 below 2^23; above, -log u = -log1p(-(1 - u)) with 1 - u = (2^24 - 1 - n + 1/2) 2^-24, again exact.
__device__ __forceinline__ float pg_gumbel(uint64_t rowkey, int i) {
#pragma clang fp contract(off)
    const uint32_t n = (uint32_t)(arl_splitmix64(rowkey ^ (uint64_t)(uint32_t)i) >> 40);
    float e;
    if (n < 0x800000u) e = -logf(((float)n + 0.5f) * (1.0f / 16777216.0f));
    else e = -log1pf(-(((float)(0xFFFFFFu - n) + 0.5f) * (1.0f / 16777216.0f)));
    return -logf(e);
}

// two running (max, sum of exp(. - max), argmax) states into one; the lower index wins an exact tie.  Symmetric in its two states bit for bit
// (contraction off), so both lanes of a butterfly pair end with the same values.
__device__ __forceinline__ void gtk_combine(float &m, float &s, int &idx, float m2, float s2, int i2) {
#pragma clang fp contract(off)
    const float M = fmaxf(m, m2);
    const float e1 = m == M ? 1.f : expf(m - M), e2 = m2 == M ? 1.f : expf(m2 - M);
    const float p1 = s * e1, p2 = s2 * e2;
    s = p1 + p2;
    if (m2 > m || (m2 == m && i2 < idx)) idx = i2;
    m = M;
}

// one workgroup per fake user, the k rounds in sequence.  dead [F][ceil(I / 32)]: the picked items' bits, cleared here before the first round.
template <bool HASH>
__global__ __launch_bounds__(kRoundsBlk) void gtk_rounds_kernel(const float *__restrict__ x, const float *__restrict__ noise, uint64_t key, int F, int I, int k,
                                                                 float tau, uint32_t *dead, int32_t *__restrict__ picks, float *__restrict__ lse,
                                                                 float *__restrict__ stats) {
#pragma clang fp contract(off)
    constexpr int NW = kRoundsBlk / 64;
    __shared__ float sm[NW], ss[NW];
    __shared__ int si[NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, f = blockIdx.x;
    const int W = (I + 31) >> 5;
    uint32_t *dd = dead + (size_t)f * W;
    for (int w = tid; w < W; w += kRoundsBlk) dd[w] = 0u;
    __threadfence_block();
    __syncthreads();
    const float *xr = x + (size_t)f * I;
    for (int r = 0; r < k; ++r) {
        const uint64_t rowkey = HASH ? pg_rowkey(key, r, f) : 0ull;
        const float *nr = HASH ? nullptr : noise + ((size_t)r * F + f) * I;
        float m = -INFINITY, s = 0.f;
        int idx = 0x7fffffff;
        for (int i = tid; i < I; i += kRoundsBlk) {
            if ((dd[i >> 5] >> (i & 31)) & 1u) continue;
            const float gn = HASH ? pg_gumbel(rowkey, i) : nr[i];
            const float z = (xr[i] + gn) / tau;
            if (z > m) { s = s * expf(m - z) + 1.f; m = z; idx = i; }            // a thread's items ascend: the first of equal values stays
            else s += expf(z - m);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) gtk_combine(m, s, idx, __shfl_xor(m, off), __shfl_xor(s, off), __shfl_xor(idx, off));
        if (lane == 0) { sm[wv] = m; ss[wv] = s; si[wv] = idx; }
        __syncthreads();
        if (wv == 0) {
            m = lane < NW ? sm[lane] : -INFINITY; s = lane < NW ? ss[lane] : 0.f; idx = lane < NW ? si[lane] : 0x7fffffff;
#pragma unroll
            for (int off = NW / 2; off > 0; off >>= 1) gtk_combine(m, s, idx, __shfl_xor(m, off), __shfl_xor(s, off), __shfl_xor(idx, off));
            if (lane == 0) {
                if ((unsigned)idx >= (unsigned)I) idx = 0;                        // only a row of NaNs gets here: stay inside the row
                const size_t o = (size_t)f * k + r;
                picks[o] = idx; lse[o] = m + logf(s); stats[2 * o] = m; stats[2 * o + 1] = s;
                dd[idx >> 5] |= 1u << (idx & 31);
            }
        }
        __threadfence_block();
        __syncthreads();
    }
}

enum { GTK_S = 0, GTK_C = 1, GTK_DX = 2 };

// one thread per (fake user, item), 256 items per workgroup, the rounds in sequence with the saved (max, sum) of every round:
//   GTK_S : out[f, i] = sum_r y_r[i]                                          (double over the rounds)
//   GTK_C : part[f][tile][r] = sum over the tile's items of y_r[i] dS[f, i]   (a wave's butterfly, the four waves in a fixed order)
//   GTK_DX: out[f, i] = (1 / tau) sum_r y_r[i] (dS[f, i] - c[f, r])
template <bool HASH, int MODE>
__global__ __launch_bounds__(kBlk) void gtk_accum_kernel(const float *__restrict__ x, const float *__restrict__ noise, uint64_t key, int F, int I, int k, float tau,
                                                          int ntiles, const int32_t *__restrict__ picks, const float *__restrict__ stats,
                                                          const float *__restrict__ dS, const float *__restrict__ c, float *__restrict__ out,
                                                          float *__restrict__ part) {
#pragma clang fp contract(off)
    __shared__ int sp[kMaxK];
    __shared__ float smx[kMaxK], ssum[kMaxK], sc[MODE == GTK_DX ? kMaxK : 1], red[MODE == GTK_C ? kWaves * kMaxK : 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int f = (int)(blockIdx.x / (unsigned)ntiles), tile = (int)(blockIdx.x % (unsigned)ntiles), i = tile * kBlk + tid;
    for (int r = tid; r < k; r += kBlk) {
        const size_t o = (size_t)f * k + r;
        sp[r] = picks[o]; smx[r] = stats[2 * o]; ssum[r] = stats[2 * o + 1];
        if (MODE == GTK_DX) sc[r] = c[o];
    }
    __syncthreads();
    const bool live = i < I;
    const int ic = live ? i : I - 1;
    const float xv = x[(size_t)f * I + ic], ds = MODE != GTK_S ? dS[(size_t)f * I + ic] : 0.f;
    bool alive = live;
    double acc = 0.0;
    for (int r = 0; r < k; ++r) {
        const float gn = HASH ? pg_gumbel(pg_rowkey(key, r, f), ic) : noise[((size_t)r * F + f) * I + ic];
        const float z = (xv + gn) / tau;
        const float y = alive ? expf(z - smx[r]) / ssum[r] : 0.f;
        if (MODE == GTK_S) acc += (double)y;
        if (MODE == GTK_C) {
            float v = y * ds;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) red[wv * kMaxK + r] = v;
        }
        if (MODE == GTK_DX) acc += (double)(y * (ds - sc[r]));
        if (sp[r] == i) alive = false;
    }
    if (MODE == GTK_C) {
        __syncthreads();
        for (int r = tid; r < k; r += kBlk)
            part[(size_t)blockIdx.x * k + r] = (red[r] + red[kMaxK + r]) + (red[2 * kMaxK + r] + red[3 * kMaxK + r]);
        return;
    }
    if (!live) return;
    out[(size_t)f * I + i] = MODE == GTK_S ? (float)acc : (float)(acc / (double)tau);
}

// c[f, r] = the tiles' partials in ascending order, in double
__global__ __launch_bounds__(kBlk) void gtk_c_kernel(const float *__restrict__ part, int k, int ntiles, float *__restrict__ c) {
    const int f = blockIdx.x;
    for (int r = threadIdx.x; r < k; r += kBlk) {
        double s = 0.0;
        for (int t = 0; t < ntiles; ++t) s += (double)part[((size_t)f * ntiles + t) * k + r];
        c[(size_t)f * k + r] = (float)s;
    }
}

__global__ __launch_bounds__(kBlk) void gtk_noise_kernel(uint64_t key, int F, int I, int ntiles, float *__restrict__ out) {
    const unsigned rf = blockIdx.x / (unsigned)ntiles, tile = blockIdx.x % (unsigned)ntiles;
    const int r = (int)(rf / (unsigned)F), f = (int)(rf % (unsigned)F), i = (int)tile * kBlk + (int)threadIdx.x;
    if (i < I) out[(size_t)rf * I + i] = pg_gumbel(pg_rowkey(key, r, f), i);
}

int gtk_shape(int64_t F, int64_t I, int64_t k, int64_t blocks_per_tile) {
    if (k > kMaxK) return ARL_E_DIM;
    if (F <= 0 || I <= 0 || k <= 0 || k > I) return ARL_E_ARG;
    if (F > 0x7fffffffll || I > kMaxI) return ARL_E_RANGE;
    if (F * blocks_per_tile * ((I + kBlk - 1) / kBlk) > 0x7fffffffll) return ARL_E_RANGE;      // one workgroup per (fake user[, round], 256 items)
    return ARL_OK;
}

}  // namespace

extern "C" {

int arl_pair_mlp_fwd_f32(const float *A, int64_t F, const float *B, int64_t I, int64_t H, const float *w2, const float *b2, float *x, arl_stream_t stream) {
    if (!A || !B || !w2 || !b2 || !x) return ARL_E_NULL;
    const int rc = pmlp_shape(F, I, H);
    if (rc != ARL_OK) return rc;
    if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)w2 | (uintptr_t)x) & 15) return ARL_E_ARG;
    hipLaunchKernelGGL(pmlp_fwd_kernel, dim3((unsigned)((I + kBlk - 1) / kBlk), (unsigned)((F + TF - 1) / TF)), dim3(kBlk), 0, (hipStream_t)stream, A, B, w2, b2, (int)F,
                       (int)I, (int)H, x);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_pair_mlp_workspace_bytes(int64_t F, int64_t I, int64_t H) {
    if (pmlp_shape(F, I, H) != ARL_OK) return 0;
    return (int64_t)(2 * up16(sizeof(double) * (size_t)pmlp_splits(F, I, H) * (size_t)F * (size_t)H) + up16(sizeof(double) * kSumBlocks));
}

int arl_pair_mlp_bwd_f32(const float *g, const float *A, int64_t F, const float *B, int64_t I, int64_t H, const float *w2, float *dA, float *dB, float *dw2,
                         float *db2, void *workspace, arl_stream_t stream) {
    if (!g || !A || !B || !w2 || !dA || !dB || !dw2 || !db2 || !workspace) return ARL_E_NULL;
    const int rc = pmlp_shape(F, I, H);
    if (rc != ARL_OK) return rc;
    if (((uintptr_t)g | (uintptr_t)A | (uintptr_t)B | (uintptr_t)w2 | (uintptr_t)dA | (uintptr_t)dB | (uintptr_t)dw2 | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int ns = pmlp_splits(F, I, H), split_len = (int)((I + ns - 1) / ns), nsum = pmlp_sum_blocks(F * I);
    const size_t slab = up16(sizeof(double) * (size_t)ns * (size_t)F * (size_t)H);
    double *partM = (double *)workspace, *partP = (double *)((char *)workspace + slab), *sum_part = (double *)((char *)workspace + 2 * slab);
    const unsigned hb = (unsigned)((H + 63) / 64);
    hipLaunchKernelGGL(pmlp_bwd_rows_kernel, dim3(hb, (unsigned)((F + TF - 1) / TF), (unsigned)ns), dim3(kBlk), 0, st, g, A, B, (int)F, (int)I, (int)H, split_len, partM,
                       partP);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pmlp_bwd_cols_kernel, dim3((unsigned)((I + kWaves * TI - 1) / (kWaves * TI)), hb), dim3(kBlk), 0, st, g, A, B, w2, (int)F, (int)I, (int)H, dB);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pmlp_sum_kernel, dim3((unsigned)nsum), dim3(kBlk), 0, st, g, (size_t)F * (size_t)I, sum_part);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pmlp_dA_kernel, dim3((unsigned)((F * H + kBlk - 1) / kBlk)), dim3(kBlk), 0, st, (const double *)partM, w2, (int)F, (int)H, ns, dA);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pmlp_finish_kernel, dim3(hb), dim3(kBlk), 0, st, (const double *)partP, (int)F, (int)H, ns, (const double *)sum_part, nsum, dw2, db2);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int64_t arl_gumbel_topk_workspace_bytes(int64_t F, int64_t I, int64_t k, int32_t backward) {
    if (gtk_shape(F, I, k, 1) != ARL_OK) return 0;
    if (!backward) return (int64_t)up16(sizeof(uint32_t) * (size_t)F * (size_t)((I + 31) / 32));
    const size_t ntiles = (size_t)((I + kBlk - 1) / kBlk);
    return (int64_t)(up16(sizeof(float) * (size_t)F * ntiles * (size_t)k) + up16(sizeof(float) * (size_t)F * (size_t)k));
}

int arl_gumbel_topk_fwd_f32(const float *x, int64_t F, int64_t I, int64_t k, float tau, const float *noise, uint64_t seed, uint64_t call, float *S, int32_t *picks,
                            float *lse, float *stats, void *workspace, arl_stream_t stream) {
    if (!x || !S || !picks || !lse || !stats || !workspace) return ARL_E_NULL;
    const int rc = gtk_shape(F, I, k, 1);
    if (rc != ARL_OK) return rc;
    if (!(tau > 0.f) || (((uintptr_t)x | (uintptr_t)noise | (uintptr_t)S | (uintptr_t)picks | (uintptr_t)lse | (uintptr_t)stats | (uintptr_t)workspace) & 15)) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t key = arl_gan_hash_key(seed, call);
    const int ntiles = (int)((I + kBlk - 1) / kBlk);
    const dim3 tiles((unsigned)(F * ntiles));
    if (noise) {
        hipLaunchKernelGGL((gtk_rounds_kernel<false>), dim3((unsigned)F), dim3(kRoundsBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, (uint32_t *)workspace, picks,
                           lse, stats);
        ARL_LAUNCH_CHECK();
        hipLaunchKernelGGL((gtk_accum_kernel<false, GTK_S>), tiles, dim3(kBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, ntiles, (const int32_t *)picks,
                           (const float *)stats, (const float *)nullptr, (const float *)nullptr, S, (float *)nullptr);
    } else {
        hipLaunchKernelGGL((gtk_rounds_kernel<true>), dim3((unsigned)F), dim3(kRoundsBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, (uint32_t *)workspace, picks,
                           lse, stats);
        ARL_LAUNCH_CHECK();
        hipLaunchKernelGGL((gtk_accum_kernel<true, GTK_S>), tiles, dim3(kBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, ntiles, (const int32_t *)picks,
                           (const float *)stats, (const float *)nullptr, (const float *)nullptr, S, (float *)nullptr);
    }
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

int arl_gumbel_topk_bwd_f32(const float *x, int64_t F, int64_t I, int64_t k, float tau, const float *noise, uint64_t seed, uint64_t call, const int32_t *picks,
                            const float *stats, const float *dS, float *dx, void *workspace, arl_stream_t stream) {
    if (!x || !picks || !stats || !dS || !dx || !workspace) return ARL_E_NULL;
    const int rc = gtk_shape(F, I, k, 1);
    if (rc != ARL_OK) return rc;
    if (!(tau > 0.f) || (((uintptr_t)x | (uintptr_t)noise | (uintptr_t)picks | (uintptr_t)stats | (uintptr_t)dS | (uintptr_t)dx | (uintptr_t)workspace) & 15)) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    const uint64_t key = arl_gan_hash_key(seed, call);
    const int ntiles = (int)((I + kBlk - 1) / kBlk);
    const dim3 tiles((unsigned)(F * ntiles));
    float *part = (float *)workspace, *c = (float *)((char *)workspace + up16(sizeof(float) * (size_t)F * (size_t)ntiles * (size_t)k));
#define GTK_BWD(HASH)                                                                                                                                  \
    do {                                                                                                                                               \
        hipLaunchKernelGGL((gtk_accum_kernel<HASH, GTK_C>), tiles, dim3(kBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, ntiles, picks, stats, dS, \
                           (const float *)nullptr, (float *)nullptr, part);                                                                            \
        ARL_LAUNCH_CHECK();                                                                                                                             \
        hipLaunchKernelGGL(gtk_c_kernel, dim3((unsigned)F), dim3(kBlk), 0, st, (const float *)part, (int)k, ntiles, c);                                \
        ARL_LAUNCH_CHECK();                                                                                                                             \
        hipLaunchKernelGGL((gtk_accum_kernel<HASH, GTK_DX>), tiles, dim3(kBlk), 0, st, x, noise, key, (int)F, (int)I, (int)k, tau, ntiles, picks, stats, dS, \
                           (const float *)c, dx, (float *)nullptr);                                                                                    \
        ARL_LAUNCH_CHECK();                                                                                                                             \
    } while (0)
    if (noise) GTK_BWD(false);
    else GTK_BWD(true);
#undef GTK_BWD
    return ARL_OK;
}

int arl_gumbel_noise_f32(uint64_t seed, uint64_t call, int64_t k, int64_t F, int64_t I, float *out, arl_stream_t stream) {
    if (!out) return ARL_E_NULL;
    if (k > kMaxK) return ARL_E_DIM;
    if (F <= 0 || I <= 0 || k <= 0) return ARL_E_ARG;
    if (F > 0x7fffffffll || I > kMaxI || F * k * ((I + kBlk - 1) / kBlk) > 0x7fffffffll) return ARL_E_RANGE;
    if ((uintptr_t)out & 15) return ARL_E_ARG;
    const int ntiles = (int)((I + kBlk - 1) / kBlk);
    hipLaunchKernelGGL(gtk_noise_kernel, dim3((unsigned)(k * F * ntiles)), dim3(kBlk), 0, (hipStream_t)stream, arl_gan_hash_key(seed, call), (int)F, (int)I, ntiles, out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

// arl_advpair.hip -- the adversarial BPR term of APR / AMF (He et al., SIGIR'18) on gfx950: BPR under the worst-case first-order perturbation of the
// rows the scorer reads, forward and backward in one call.
//
// Batch u, p, n [B]; positions t = b (user of sample b), B + b (its positive), 2B + b (its negative); row(t) = where position t's row is READ
// (u[b], item_off + p[b], item_off + n[b]); group(t) = which NODE it is (groups[t]; NULL: row(t), or t itself with distinct_rows).
//   Gamma_g = sum over the positions of group g, in ascending t, of d bpr / d (that position's row)         (the clean BPR's gradient per node)
//   delta_g = eps * Gamma_g / sqrt(max(|Gamma_g|^2, 1e-12))                                                  (row-wise l2_normalize; 0 stays 0)
//   adv     = mean_b -log(10e-8 + sigmoid(<u', p'> - <u', n'>)),  x' = x + delta_group(x)                    (delta is a constant of the step)
//   G[row(t)] += upstream * d adv / d (position t's row), duplicates in ascending t on top of what G holds   (no float atomics)
// Four launches, each one wave per sample or per position; a launch boundary is the only hand-off between them:
//   1 adv_clean_kernel   sample:    clean score, coefficient c_b = -s (1 - s) / (10e-8 + s) / B, loss term
//   2 adv_delta_kernel   position:  the first position of a group owns it (ordered_scan_lds over the 3B group ids): Gamma, delta, owner[]
//   3 adv_pert_kernel    sample:    perturbed score, coefficient c'_b, loss term (and the per-position delta_out)
//   4 adv_bwd_kernel     position:  the first position of a ROW owns it: the ordered backward; one more workgroup reduces both losses (fixed tree)
// Gamma must be complete before any delta exists, so the list is one window: 3B <= kOrderedWindow.
// workspace (4-byte words): c[B] | term[B] | c'[B] | term'[B] | owner[3B] (int32) | delta[3B][d] (an owner's slot holds its group's delta; the
// other slots are never written and never read).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "arlib_amd.h"
#include "arl_util.h"
#include "arl_ordered.h"

// a + (-a) must cancel exactly (a sample with p == n leaves its item's Gamma at 0): no product is fused into the sum that follows it
#pragma clang fp contract(off)

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr int kMaxWidth = 256;               // a lane holds columns lane, 64 + lane, 128 + lane, 192 + lane

__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off);
    return v;
}

struct AdvBatch {
    const float *emb;
    const int32_t *ui, *pi, *ni, *groups;
    long long item_off;
    int d, B, distinct;
    __device__ __forceinline__ long long row(int t) const {
        return t < B ? (long long)ui[t] : (t < 2 * B ? item_off + pi[t - B] : item_off + ni[t - 2 * B]);
    }
    __device__ __forceinline__ int group(int t) const { return groups ? groups[t] : (distinct ? t : (int)row(t)); }
};

struct AdvWs {
    float *c, *term, *c2, *term2, *delta;
    int32_t *owner;
};

__host__ __device__ inline AdvWs adv_ws(void *base, int64_t B, int64_t d) {
    AdvWs w;
    float *f = (float *)base;
    w.c = f; w.term = f + B; w.c2 = f + 2 * B; w.term2 = f + 3 * B;
    w.owner = (int32_t *)(f + 4 * B);
    w.delta = f + 7 * B;
    return w;
}

// x = <u, p> - <u, n> of one sample -> (d mean loss / dx, the sample's loss term), written by lane 0.  One lane per sample: the sigmoid and the
// logarithm run in double (the fp32 expf / logf are a few ulp off, which is the whole error of a loss term) and are rounded once.
__device__ __forceinline__ void adv_score(float ps, float ns, float b_norm, float *c, float *term, int b, int lane) {
    ps = wave_sum(ps); ns = wave_sum(ns);
    if (lane == 0) {
        const double x = (double)(ps - ns);
        const double s = 1.0 / (1.0 + exp(-x));
        c[b] = (float)(-(s * (1.0 - s)) / ((1e-7 + s) * (double)b_norm));
        term[b] = (float)(-log(1e-7 + s));
    }
}

__global__ __launch_bounds__(kBlk) void adv_clean_kernel(AdvBatch a, AdvWs w) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= a.B) return;
    const float *u = a.emb + (size_t)a.row(b) * a.d, *p = a.emb + (size_t)a.row(a.B + b) * a.d, *n = a.emb + (size_t)a.row(2 * a.B + b) * a.d;
    float ps = 0.f, ns = 0.f;
    for (int k = lane; k < a.d; k += 64) {
        const float uk = u[k];
        ps = fmaf(uk, p[k], ps); ns = fmaf(uk, n[k], ns);
    }
    adv_score(ps, ns, (float)a.B, w.c, w.term, b, lane);
}

__global__ __launch_bounds__(kBlk) void adv_delta_kernel(AdvBatch a, AdvWs w, float eps) {
    extern __shared__ int32_t sgrp[];
    const int lane = threadIdx.x & 63, T = 3 * a.B, d = a.d, B = a.B;
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const bool scan = a.groups || !a.distinct;                  // otherwise every position is its own group
    if (scan) {
        for (int j = threadIdx.x; j < T; j += kBlk) sgrp[j] = a.group(j);
        __syncthreads();
    }
    if (t >= T) return;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    auto term = [&](int tt) {
        if (tt >= T) return;                                    // (a negative group id would match the scan's padding)
        const int kind = tt / B, b = tt - kind * B;
        const float c = w.c[b];
        if (lane == 0) w.owner[tt] = t;
        const float *x = a.emb + (size_t)(kind == 0 ? a.row(B + b) : a.row(b)) * d;      // the partner: positive row (user term) / user row (item terms)
        const float *y = a.emb + (size_t)a.row(2 * B + b) * d;                           // negative row (user term only)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 64 * i + lane;
            if (k < d) acc[i] += kind == 0 ? c * (x[k] - y[k]) : (kind == 1 ? c * x[k] : -(c * x[k]));
        }
    };
    if (!scan) term(t);
    else if (!ordered_scan_lds(sgrp, 0, T, t, a.group(t), lane, term)) return;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) ss = fmaf(acc[i], acc[i], ss);
    const float sc = eps / sqrtf(fmaxf(wave_sum(ss), 1e-12f));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = 64 * i + lane;
        if (k < d) w.delta[(size_t)t * d + k] = sc * acc[i];
    }
}

__global__ __launch_bounds__(kBlk) void adv_pert_kernel(AdvBatch a, AdvWs w, float *__restrict__ delta_out) {
    const int lane = threadIdx.x & 63, B = a.B, d = a.d;
    const int b = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (b >= B) return;
    const float *u = a.emb + (size_t)a.row(b) * d, *p = a.emb + (size_t)a.row(B + b) * d, *n = a.emb + (size_t)a.row(2 * B + b) * d;
    const float *du = w.delta + (size_t)w.owner[b] * d, *dp = w.delta + (size_t)w.owner[B + b] * d, *dn = w.delta + (size_t)w.owner[2 * B + b] * d;
    float ps = 0.f, ns = 0.f;
    for (int k = lane; k < d; k += 64) {
        const float eu = du[k], ep = dp[k], en = dn[k];
        const float uk = u[k] + eu;
        ps = fmaf(uk, p[k] + ep, ps); ns = fmaf(uk, n[k] + en, ns);
        if (delta_out) {
            delta_out[(size_t)b * d + k] = eu; delta_out[(size_t)(B + b) * d + k] = ep; delta_out[(size_t)(2 * B + b) * d + k] = en;
        }
    }
    adv_score(ps, ns, (float)B, w.c2, w.term2, b, lane);
}

// the last workgroup: loss_out = [mean of term', mean of term], in double: a thread's strided terms and then a tree over the workgroup
__global__ __launch_bounds__(kBlk) void adv_bwd_kernel(AdvBatch a, AdvWs w, float upstream, float *__restrict__ G, float *__restrict__ loss_out) {
    extern __shared__ __attribute__((aligned(16))) int32_t srows[];
    const int lane = threadIdx.x & 63, T = 3 * a.B, d = a.d, B = a.B;
    if (blockIdx.x == gridDim.x - 1) {
        double *sh = reinterpret_cast<double *>(srows);
        double s0 = 0.0, s1 = 0.0;
        for (int i = threadIdx.x; i < B; i += kBlk) { s0 += (double)w.term2[i]; s1 += (double)w.term[i]; }
        sh[threadIdx.x] = s0; sh[kBlk + threadIdx.x] = s1;
        __syncthreads();
        for (int s = kBlk / 2; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) { sh[threadIdx.x] += sh[threadIdx.x + s]; sh[kBlk + threadIdx.x] += sh[kBlk + threadIdx.x + s]; }
            __syncthreads();
        }
        if (threadIdx.x == 0) { loss_out[0] = (float)(sh[0] / (double)B); loss_out[1] = (float)(sh[kBlk] / (double)B); }
        return;
    }
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (!a.distinct) {
        for (int j = threadIdx.x; j < T; j += kBlk) srows[j] = (int32_t)a.row(j);
        __syncthreads();
    }
    if (t >= T) return;
    const int row = (int)a.row(t);
    float *o = G + (size_t)row * d;
    float acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = 64 * i + lane; acc[i] = k < d ? o[k] : 0.f; }
    auto term = [&](int tt) {
        if (tt >= T) return;
        const int kind = tt / B, b = tt - kind * B;
        const float g = w.c2[b] * upstream;
        const int tx = kind == 0 ? B + b : b, ty = 2 * B + b;                           // the partner positions, as in adv_delta_kernel
        const float *x = a.emb + (size_t)a.row(tx) * d, *dx = w.delta + (size_t)w.owner[tx] * d;
        const float *y = a.emb + (size_t)a.row(ty) * d, *dy = w.delta + (size_t)w.owner[ty] * d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 64 * i + lane;
            if (k < d) {
                const float xp = x[k] + dx[k];
                acc[i] += kind == 0 ? g * (xp - (y[k] + dy[k])) : (kind == 1 ? g * xp : -(g * xp));
            }
        }
    };
    // distinct: the caller guarantees 3B distinct rows (compact batch form) -- every position owns its row, a plain store-add
    if (a.distinct) term(t);
    else if (!ordered_scan_lds(srows, 0, T, t, row, lane, term)) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) { const int k = 64 * i + lane; if (k < d) o[k] = acc[i]; }
}

bool adv_shape(int64_t B, int64_t d) { return B >= 1 && 3 * B <= kOrderedWindow && d >= 1 && d <= kMaxWidth; }

}  // namespace

extern "C" {

int64_t arl_bpr_adv_workspace_bytes(int64_t B, int64_t d) {
    if (!adv_shape(B, d)) return 0;
    return ((int64_t)sizeof(float) * (7 * B + 3 * B * d) + 15) / 16 * 16;
}

int arl_bpr_adv_fwd_bwd_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p, const int32_t *n, int64_t B,
                            const int32_t *groups, float eps, float upstream, float *loss_out, float *G, float *delta_out, void *workspace,
                            int32_t distinct_rows, arl_stream_t stream) {
    if (!emb || !u || !p || !n || !loss_out || !workspace) return ARL_E_NULL;
    if (B <= 0 || item_off < 0 || !(eps >= 0.f)) return ARL_E_ARG;
    if (d <= 0 || d > kMaxWidth) return ARL_E_DIM;
    if (3 * B > kOrderedWindow) return ARL_E_RANGE;
    hipStream_t st = (hipStream_t)stream;
    const AdvBatch a{emb, u, p, n, groups, (long long)item_off, (int)d, (int)B, distinct_rows != 0};
    const AdvWs w = adv_ws(workspace, B, d);
    const unsigned gs = (unsigned)((B + kWaves - 1) / kWaves), gp = (unsigned)((3 * B + kWaves - 1) / kWaves);
    const size_t list = (size_t)(3 * B) * sizeof(int32_t), red = (size_t)2 * kBlk * sizeof(double);
    hipLaunchKernelGGL(adv_clean_kernel, dim3(gs), dim3(kBlk), 0, st, a, w);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(adv_delta_kernel, dim3(gp), dim3(kBlk), (groups || !distinct_rows) ? list : 0, st, a, w, eps);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(adv_pert_kernel, dim3(gs), dim3(kBlk), 0, st, a, w, delta_out);
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL(adv_bwd_kernel, dim3((G ? gp : 0u) + 1u), dim3(kBlk), (!distinct_rows && list > red) ? list : red, st, a, w, upstream, G, loss_out);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // extern "C"

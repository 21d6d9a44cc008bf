// arl_targetrank.hip -- the rank of each target item for each user over the whole catalogue, on gfx950 without the U x I
// score matrix.  With s = Pu Pi^T as the kernels compute it:
//     rank[u, t] = #{ j != targets[t], (u, j) not masked :  s[u, j] > s[u, targets[t]]  or  (s[u, j] == s[u, targets[t]] and j < targets[t]) },
// the 0-based position of the target in a descending sort of user u's row with ties broken by item id; -1 where (u, targets[t]) is itself masked.
// The reference's AttackMetric (util/metrics.py:125-208) reads only `rank < k` and `disc[rank]`, so this matrix serves all of its numbers at any k.
//
// Rules kept throughout (the streamed tile is the shared one of arl_stream.h):
//   * every score is the exact fp32 contraction on v_mfma_f32_16x16x4_f32, and every score that feeds a comparison comes off the SAME instruction
//     sequence (strm::scores / strm::scores4; the stream's TRK_MFMA4 is the same): the thresholds (pass 1), the stream (pass 2) and the gathered scores of the correction (pass 3).  The
//     matrix core computes each output element as its own k-ordered fmaf chain, so the score of a pair (u, j) has the same bits in all three.
//   * pass 1: tscore[u, t] = s[u, targets[t]], the single producer of every threshold;
//   * pass 2: users resident (16 per wave in registers), items streamed through LDS in 64-row double-buffered stages (optionally in splits of the
//     item range); the epilogue turns each score into an order-preserving integer key and adds `key > eff[t]` to TG integer counters per lane.
//     eff[t] is key(threshold) - 1 up to and including the 64-item stage that holds targets[t] (counting >=, the rule for items before the target)
//     and key(threshold) after it (counting >): one integer compare and one add per score and target, no item index in the inner loop;
//   * pass 3, a wave per user: re-scores the target's own stage from the target on and takes back what pass 2 counted there against the rule (the
//     target itself, by index, and later items that tie), then gathers the masked items of the row, subtracts those that beat each threshold and
//     writes -1 where the target is listed; folds the splits.
//   * integer counters only: any order gives the same bits.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include "arlib_amd.h"
#include "arl_stream.h"

namespace {

constexpr int kBlk = 256, kWaves = 4;
constexpr int kMaxTargets = 64;
using strm::f32x4v;

// an int32 that orders as the float does (finite values and infinities); the two zeros share a key
__device__ __forceinline__ int trk_key(float s) {
    int b = __float_as_int(s);
    b = b == INT_MIN ? 0 : b;
    return b ^ ((b >> 31) & 0x7fffffff);
}

// Pass 1.  A wave keeps 16 users; the target rows are the A operand straight from memory.  tscore [nU, T].
template <int D>
__global__ __launch_bounds__(kBlk) void trk_thresh_kernel(const float *__restrict__ Pu, int nU, const float *__restrict__ Pi, const int32_t *__restrict__ targets, int T,
                                                           float *__restrict__ tscore) {
    constexpr int Q = D / 4;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    if (r0 >= nU) return;                                                // the whole wave leaves
    float br[Q];
    strm::load_resident<D>(Pu, min(r0 + c, nU - 1), nU, g, br);
    for (int sub = 0; sub * 16 < T; ++sub) {
        const int item = targets[min(sub * 16 + c, T - 1)];
        const f32x4v sc = strm::scores<D>(Pi + (size_t)item * D + Q * g, br);
        if (r0 + c < nU) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int t = sub * 16 + 4 * g + j;
                if (t < T) tscore[(size_t)(r0 + c) * T + t] = sc[j];
            }
        }
    }
}

// This kernel keeps its own copy of the shared tile (arl_stream.h: load_resident, stage<D>, scores4): built from the shared pieces, <64, 16> measured
// 0.3 % slower at 1 M x 100 K (370.0 against 369.0 ms, five runs each, this copy's own run-to-run spread 0.5 %) while <64, 32> and <64, 64> measured 0.2 - 0.5 %
// faster; the instruction mix was the same, the schedule was not.  TRK_MFMA4 is strm::scores' sequence.
#define TRK_MFMA4(SC, A, BR, I)                                                  \
    do {                                                                         \
        SC = __builtin_amdgcn_mfma_f32_16x16x4f32((A).x, BR[(I)], SC, 0, 0, 0);     \
        SC = __builtin_amdgcn_mfma_f32_16x16x4f32((A).y, BR[(I) + 1], SC, 0, 0, 0); \
        SC = __builtin_amdgcn_mfma_f32_16x16x4f32((A).z, BR[(I) + 2], SC, 0, 0, 0); \
        SC = __builtin_amdgcn_mfma_f32_16x16x4f32((A).w, BR[(I) + 3], SC, 0, 0, 0); \
    } while (0)
// Pass 2.  part [gridDim.y][nU][T]: the counts of the split's items under the stage rule above.  split_len is a multiple of 64.
template <int D, int TG>
__global__ __launch_bounds__(kBlk) void trk_stream_kernel(const float *__restrict__ Pu, int nU, const float *__restrict__ Pi, int nI, int split_len,
                                                           const int32_t *__restrict__ targets, int T, const float *__restrict__ tscore, int32_t *__restrict__ part) {
    constexpr int Q = D / 4, LD = D + 4;
    __shared__ float tile[2][64 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, g = lane >> 4;
    const int r0 = (blockIdx.x * kWaves + wv) * 16;
    const int t_begin = blockIdx.y * split_len, t_end = min(nI, t_begin + split_len);
    float br[Q];
    {
        const int r = r0 + c;
#pragma unroll
        for (int i = 0; i < Q; i += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < nU) v = *reinterpret_cast<const float4 *>(Pu + (size_t)r * D + Q * g + i);
            br[i] = v.x; br[i + 1] = v.y; br[i + 2] = v.z; br[i + 3] = v.w;
        }
    }
    int eff[TG], cnt[TG];
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        cnt[t] = 0;
        const int tc = min(t, T - 1);
        const float v = tscore[(size_t)min(r0 + c, nU - 1) * T + tc];
        const int e = trk_key(v) - ((targets[tc] >> 6) >= (t_begin >> 6) ? 1 : 0);
        eff[t] = t < T ? e : INT_MAX;                                    // a slot past T never counts
    }
    const int nst = max(0, (t_end - t_begin + 63) / 64);
    constexpr int PF = 64 * (D / 4) / kBlk;
    f32x4v pre[PF];
    const int frow = tid / (D / 4), fq = (tid % (D / 4)) * 4;
    constexpr int FSTEP = kBlk / (D / 4);
#define TRK_FETCH(ST)                                                                                                              \
    do {                                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < PF; ++i) {                                                                           \
            const int t = min(t_begin + (ST) * 64 + frow + i * FSTEP, nI - 1);     /* clamped; rows past t_end are masked below */ \
            pre[i] = *reinterpret_cast<const f32x4v *>(Pi + (size_t)t * D + fq);                                                   \
        }                                                                                                                          \
    } while (0)
#define TRK_STASH(BUF)                                                                                                             \
    do {                                                                                                                           \
        _Pragma("unroll") for (int i = 0; i < PF; ++i) *reinterpret_cast<f32x4v *>(&tile[BUF][(frow + i * FSTEP) * LD + fq]) = pre[i]; \
    } while (0)
    if (nst > 0) { TRK_FETCH(0); TRK_STASH(0); }
    __syncthreads();
    for (int st = 0; st < nst; ++st) {
        const int buf = st & 1;
        if (st + 1 < nst) TRK_FETCH(st + 1);
        const float *Tl = tile[buf];
        // the stage's four 16-row tiles as four independent accumulator chains
        f32x4v sc0 = f32x4v{0.f, 0.f, 0.f, 0.f}, sc1 = sc0, sc2 = sc0, sc3 = sc0;
        const float *arow = Tl + c * LD + Q * g;
#pragma unroll
        for (int i = 0; i < Q; i += 4) {
            const float4 a0 = *reinterpret_cast<const float4 *>(arow + i);
            const float4 a1 = *reinterpret_cast<const float4 *>(arow + 16 * LD + i);
            const float4 a2 = *reinterpret_cast<const float4 *>(arow + 32 * LD + i);
            const float4 a3 = *reinterpret_cast<const float4 *>(arow + 48 * LD + i);
            TRK_MFMA4(sc0, a0, br, i);
            TRK_MFMA4(sc1, a1, br, i);
            TRK_MFMA4(sc2, a2, br, i);
            TRK_MFMA4(sc3, a3, br, i);
        }
        const int sb = t_begin + st * 64 + 4 * g;                        // item of tile 0, register 0
        int k[16];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            k[j] = sb + j < t_end ? trk_key(sc0[j]) : INT_MIN;           // INT_MIN is below every eff: a row past the end never counts
            k[4 + j] = sb + 16 + j < t_end ? trk_key(sc1[j]) : INT_MIN;
            k[8 + j] = sb + 32 + j < t_end ? trk_key(sc2[j]) : INT_MIN;
            k[12 + j] = sb + 48 + j < t_end ? trk_key(sc3[j]) : INT_MIN;
        }
        const int stage = (t_begin >> 6) + st;
#pragma unroll
        for (int t = 0; t < TG; ++t) {
#pragma unroll
            for (int q = 0; q < 16; ++q) cnt[t] += k[q] > eff[t] ? 1 : 0;
            // past the target's stage: from >= to > (a clamped read and a uniform flag, no branch; a slot past T stays at INT_MAX)
            eff[t] += (t < T && (targets[min(t, T - 1)] >> 6) == stage) ? 1 : 0;
        }
        if (st + 1 < nst) TRK_STASH(buf ^ 1);
        __syncthreads();
    }
#undef TRK_FETCH
#undef TRK_STASH
#undef TRK_MFMA4
    // the four lane groups of a resident row hold disjoint items
#pragma unroll
    for (int t = 0; t < TG; ++t) {
        cnt[t] += __shfl_xor(cnt[t], 16);
        cnt[t] += __shfl_xor(cnt[t], 32);
    }
    if (g == 0 && r0 + c < nU) {
        int32_t *dst = part + ((size_t)blockIdx.y * nU + (r0 + c)) * T;
#pragma unroll
        for (int t = 0; t < TG; ++t)
            if (t < T) dst[t] = cnt[t];
    }
}

// Pass 3, a wave per user u.  Scores 64 gathered item rows at a time against the user's row (the B operand holds it in all 16 columns, so every
// column of the tile carries the same 16 scores); lane (c, g) owns targets c, c + 16, c + 32, c + 48 and sees rows 16 sub + 4 g + j of each tile.
// part may be rank itself (n_splits = 1: the stream wrote its counts there), so neither is __restrict__.
template <int D>
__global__ __launch_bounds__(kBlk) void trk_finish_kernel(const float *__restrict__ Pu, int nU, const float *__restrict__ Pi, int nI, const int32_t *__restrict__ targets,
                                                           int T, const float *__restrict__ tscore, const int32_t *__restrict__ mptr,
                                                           const int32_t *__restrict__ mcol, const int32_t *part, int n_splits, int32_t *rank) {
    constexpr int Q = D / 4, TT = kMaxTargets / 16;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, c = lane & 15, g = lane >> 4;
    const int u = blockIdx.x * kWaves + wv;
    if (u >= nU) return;                                                 // the whole wave leaves
    float br[Q];
    strm::load_resident<D>(Pu, u, nU, g, br);
    int tgt[TT], key[TT], take[TT], listed[TT];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int t = c + 16 * tt;
        tgt[tt] = t < T ? targets[t] : -1;
        key[tt] = t < T ? trk_key(tscore[(size_t)u * T + t]) : INT_MAX;
        take[tt] = 0;
        listed[tt] = 0;
    }
    // scores of the rows it0..it3 (one per tile, this lane's row 16 sub + c) against the user's row
#define TRK_SCORE64(IT0, IT1, IT2, IT3)                                                                                               \
    f32x4v sc[4];                                                                                                                     \
    strm::scores4<D>(Pi + (size_t)(IT0) * D + Q * g, Pi + (size_t)(IT1) * D + Q * g, Pi + (size_t)(IT2) * D + Q * g, Pi + (size_t)(IT3) * D + Q * g, br, sc);
    // (a) the target's own 64-item stage, where the stream counted >= for every item: take back the target itself (by index) and the later ties
    for (int t = 0; t < T; ++t) {
        const int tg = targets[t], s0 = (tg >> 6) << 6;
        const int kt = trk_key(tscore[(size_t)u * T + t]);
        const int i0 = min(s0 + c, nI - 1), i1 = min(s0 + 16 + c, nI - 1), i2 = min(s0 + 32 + c, nI - 1), i3 = min(s0 + 48 + c, nI - 1);
        TRK_SCORE64(i0, i1, i2, i3)
        int v = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int item = s0 + 4 * g + j;
            const int k0 = trk_key(sc[0][j]), k1 = trk_key(sc[1][j]), k2 = trk_key(sc[2][j]), k3 = trk_key(sc[3][j]);
#define TRK_OWN(ITEM, K) (((ITEM) < nI) && ((ITEM) == tg ? (K) >= kt : ((ITEM) > tg && (K) == kt)) ? 1 : 0)
            v += TRK_OWN(item, k0) + TRK_OWN(item + 16, k1) + TRK_OWN(item + 32, k2) + TRK_OWN(item + 48, k3);
#undef TRK_OWN
        }
        if (c == (t & 15)) {
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) take[tt] += tt == (t >> 4) ? v : 0;
        }
    }
    // (b) the masked items of the row: those that beat a threshold leave its count; a listed target makes the pair invalid
    if (mptr) {
        const int k_begin = mptr[u], k_end = mptr[u + 1];
        for (int kb = k_begin; kb < k_end; kb += 64) {
            const int last = k_end - 1;
            const int i0 = mcol[min(kb + c, last)], i1 = mcol[min(kb + 16 + c, last)], i2 = mcol[min(kb + 32 + c, last)], i3 = mcol[min(kb + 48 + c, last)];
            TRK_SCORE64(i0, i1, i2, i3)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 4 * g + j;                               // lane `row` (c = row, g = 0) fetched this row's item of every tile
                const int it[4] = {__shfl(i0, row), __shfl(i1, row), __shfl(i2, row), __shfl(i3, row)};
                const int kk[4] = {trk_key(sc[0][j]), trk_key(sc[1][j]), trk_key(sc[2][j]), trk_key(sc[3][j])};
#pragma unroll
                for (int sub = 0; sub < 4; ++sub) {
                    const bool live = kb + 16 * sub + row < k_end;
#pragma unroll
                    for (int tt = 0; tt < TT; ++tt) {
                        const bool beats = it[sub] != tgt[tt] && kk[sub] > key[tt] - (it[sub] < tgt[tt] ? 1 : 0);
                        take[tt] += live && beats ? 1 : 0;
                        listed[tt] |= live && it[sub] == tgt[tt] ? 1 : 0;
                    }
                }
            }
        }
    }
#undef TRK_SCORE64
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        take[tt] += __shfl_xor(take[tt], 16);
        take[tt] += __shfl_xor(take[tt], 32);
        listed[tt] |= __shfl_xor(listed[tt], 16);
        listed[tt] |= __shfl_xor(listed[tt], 32);
    }
    if (g != 0) return;
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int t = c + 16 * tt;
        if (t >= T) continue;
        const size_t e = (size_t)u * T + t, stride = (size_t)nU * T;
        int total = part[e];
        for (int s = 1; s < n_splits; ++s) total += part[(size_t)s * stride + e];
        rank[e] = listed[tt] ? -1 : total - take[tt];
    }
}

// splits of the item stream when the user side is short: enough workgroups to fill the chip a few times over, at least 512 items each, whole stages
void trk_splits(int64_t U, int64_t I, int *n_splits, int *split_len) {
    const int64_t row_blocks = (U + 63) / 64;
    int64_t s = (1024 + row_blocks - 1) / row_blocks;
    const int64_t max_s = (I + 511) / 512;
    if (s > max_s) s = max_s;
    if (s > 64) s = 64;
    if (s < 1) s = 1;
    const int64_t len = ((I + s - 1) / s + 63) / 64 * 64;
    *split_len = (int)len;
    *n_splits = (int)((I + len - 1) / len);
}

bool trk_shape_ok(int64_t U, int64_t I, int64_t d, int64_t T) {
    return strm::shape_ok(U, I, d) && T >= 1 && T <= kMaxTargets;
}

template <int D>
int trk_run(const float *Pu, int64_t U, const float *Pi, int64_t I, const int32_t *targets, int T, const int32_t *mptr, const int32_t *mcol, int32_t *rank,
            float *tscore, char *ws, hipStream_t st) {
    const dim3 blk(kBlk);
    const unsigned row_blocks = (unsigned)((U + 63) / 64);
    int ns, split_len;
    trk_splits(U, I, &ns, &split_len);
    int32_t *part = ns > 1 ? (int32_t *)ws : rank;
    hipLaunchKernelGGL((trk_thresh_kernel<D>), dim3(row_blocks), blk, 0, st, Pu, (int)U, Pi, targets, T, tscore);
    ARL_LAUNCH_CHECK();
    const dim3 grid(row_blocks, (unsigned)ns);
#define TRK_STREAM(TG) hipLaunchKernelGGL((trk_stream_kernel<D, TG>), grid, blk, 0, st, Pu, (int)U, Pi, (int)I, split_len, targets, T, (const float *)tscore, part)
    if (T <= 8) TRK_STREAM(8);
    else if (T <= 16) TRK_STREAM(16);
    else if (T <= 32) TRK_STREAM(32);
    else TRK_STREAM(64);
#undef TRK_STREAM
    ARL_LAUNCH_CHECK();
    hipLaunchKernelGGL((trk_finish_kernel<D>), dim3((unsigned)((U + kWaves - 1) / kWaves)), blk, 0, st, Pu, (int)U, Pi, (int)I, targets, T, (const float *)tscore, mptr, mcol,
                       (const int32_t *)part, ns, rank);
    ARL_LAUNCH_CHECK();
    return ARL_OK;
}

}  // namespace

extern "C" {

int64_t arl_target_rank_workspace_bytes(int64_t U, int64_t I, int64_t d, int64_t T) {
    if (!trk_shape_ok(U, I, d, T)) return 0;
    int ns, split_len;
    trk_splits(U, I, &ns, &split_len);
    return ns > 1 ? (int64_t)up16(sizeof(int32_t) * (size_t)ns * (size_t)U * (size_t)T) : 0;
}

int arl_target_rank_f32(const float *Pu, int64_t U, const float *Pi, int64_t I, int64_t d, const int32_t *targets, int64_t T, const int32_t *mask_rowptr,
                        const int32_t *mask_col, int32_t *rank, float *tscore, void *workspace, arl_stream_t stream) {
    if (!Pu || !Pi || !targets || !rank || !tscore || !workspace) return ARL_E_NULL;
    if ((mask_rowptr == nullptr) != (mask_col == nullptr)) return ARL_E_NULL;
    if (!trk_shape_ok(U, I, d, T)) return ARL_E_RANGE;
    if (((uintptr_t)Pu | (uintptr_t)Pi | (uintptr_t)workspace) & 15) return ARL_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace;
#define TRK_RUN(DD) return trk_run<DD>(Pu, U, Pi, I, targets, (int)T, mask_rowptr, mask_col, rank, tscore, ws, st)
    ARL_DISPATCH_WIDTH(d, TRK_RUN);
#undef TRK_RUN
}

}  // extern "C"

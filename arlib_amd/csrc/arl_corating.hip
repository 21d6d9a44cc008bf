// arl_corating.hip -- GOAT's co-rating degree (reference attack/Gray/GOAT.py:37-39) on gfx950.
//
// The reference forms interact.T @ interact (I x I, close to dense on a large catalogue), sets every stored entry to 1 and sums the columns:
// itemIntNum[j] = the number of items that share at least one user with item j (j itself included, 0 for an item nobody rated).  Here the
// product is never formed.  A workgroup owns one item j and a bitmap of I bits in LDS: it clears the bitmap, ORs the bits of every item of every
// user of j into it (one wave per user, the user's row read coalesced, ds_or_b32 on the word), and after a barrier popcounts the words.
//
// Rules kept:
//   * integer result, exact and independent of the order of the ORs: bit-identical from run to run;
//   * the bitmap and the four wave partials are the kernel's only scratch, both in dynamic LDS and both written before they are read; the only
//     global write is out[j], by thread 0 of the item's workgroup: every out[j] is written exactly once, whatever `order` is (a permutation);
//   * an item without users writes 0 and returns before it touches LDS;
//   * block b takes item order[b] (heaviest first, so a hub does not form the tail of the launch), or item b when order is NULL;
//   * an item id outside [0, n_items) in `col` is skipped, never turned into an LDS address.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "arlib_amd.h"

namespace {

constexpr int kBlk = 256, kWaves = kBlk / 64;
constexpr int kHeadWords = 16;                                  // the wave partials, padded to 64 bytes in front of the bitmap
constexpr int64_t kLdsBytes = 160 * 1024;                       // LDS of one CU of gfx950: one workgroup may take all of it
constexpr int64_t kMaxWords = kLdsBytes / 4 - kHeadWords;
constexpr int64_t kMaxItems = kMaxWords * 32;

__global__ __launch_bounds__(kBlk) void corating_degree_kernel(const int64_t *__restrict__ u_rowptr, const int32_t *__restrict__ u_col,
                                                                const int64_t *__restrict__ i_colptr, const int32_t *__restrict__ i_row,
                                                                const int32_t *__restrict__ order, int n_users, int n_items,
                                                                int32_t *__restrict__ out) {
    extern __shared__ uint32_t lds[];
    uint32_t *part = lds, *bits = lds + kHeadWords;
    const int j = order ? order[blockIdx.x] : (int)blockIdx.x;
    if ((unsigned)j >= (unsigned)n_items) return;               // `order` is a permutation; anything else is dropped, not dereferenced
    const int64_t ub = i_colptr[j], ue = i_colptr[j + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (ue <= ub) {                                             // uniform over the workgroup: no barrier is skipped by part of it
        if (tid == 0) out[j] = 0;
        return;
    }
    const int words = (n_items + 31) >> 5;
    for (int w = tid; w < words; w += kBlk) bits[w] = 0u;
    __syncthreads();
    for (int64_t p = ub + wv; p < ue; p += kWaves) {
        const int u = i_row[p];
        if ((unsigned)u >= (unsigned)n_users) continue;
        const int64_t b = u_rowptr[u], e = u_rowptr[u + 1];
        for (int64_t q = b + lane; q < e; q += 64) {
            const int i = u_col[q];
            if ((unsigned)i < (unsigned)n_items) atomicOr(&bits[i >> 5], 1u << (i & 31));
        }
    }
    __syncthreads();
    int cnt = 0;
    for (int w = tid; w < words; w += kBlk) cnt += __popc(bits[w]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
    if (lane == 0) part[wv] = (uint32_t)cnt;
    __syncthreads();
    if (tid == 0) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) s += (int)part[w];
        out[j] = s;
    }
}

}  // namespace

extern "C" {

int64_t arl_corating_max_items(void) { return kMaxItems; }

int arl_corating_degree_i32(const int64_t *u_rowptr, const int32_t *u_col, const int64_t *i_colptr, const int32_t *i_row, int64_t n_users,
                            int64_t n_items, const int32_t *order, int32_t *out, arl_stream_t stream) {
    if (n_users < 0 || n_items < 0) return ARL_E_ARG;
    if (n_items > kMaxItems || n_users > 0x7fffffffll) return ARL_E_RANGE;
    if (n_items == 0) return ARL_OK;
    if (!u_rowptr || !i_colptr || !out) return ARL_E_NULL;      // u_col / i_row may be NULL for a matrix without entries
    const int64_t words = (n_items + 31) / 32;
    const size_t shm = sizeof(uint32_t) * (size_t)(kHeadWords + words);
    if (shm > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)corating_degree_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)shm);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(corating_degree_kernel, dim3((unsigned)n_items), dim3(kBlk), shm, (hipStream_t)stream, u_rowptr, u_col, i_colptr, i_row, order,
                       (int)n_users, (int)n_items, out);
    hipError_t e = hipGetLastError();
    return e != hipSuccess ? (int)e : ARL_OK;
}

}  // extern "C"

// arl_stream.h -- the streamed score tile every "streaming" kernel of the library is built from ("the shared tile").
//
// A workgroup of 256 threads (four waves) scores 64 rows of a RESIDENT table against a STREAMED table on v_mfma_f32_16x16x4_f32 and never stores
// the scores:
//   * lane (c, g) = (lane & 15, lane >> 4) of a wave keeps columns [D/4 g, D/4 (g + 1)) of resident row r0 + c in br[D/4] (the B operand; a
//     permutation of the contraction index both operands share);
//   * the streamed table passes through LDS 64 rows a stage, row stride D + 4 floats (the four lane groups read four disjoint bank quarters),
//     double-buffered: the NEXT stage is fetched into registers before the current one is consumed and goes to the other buffer afterwards, one
//     barrier per stage;
//   * the 16 x 16 score tile `sub` of a stage comes out as C[t = 4 g + reg][r = c]: register j of lane (c, g) is streamed row 16 sub + 4 g + j
//     against resident row r0 + c, which is already the A-operand layout of the second product out[r][:] += sum_t w[t][r] Xt[t][:].
// Each family keeps its own __global__ kernel, loop and epilogue and calls these pieces; nothing here belongs to one family.  The pieces hold
// only loads, stores and MFMA builtins (and one sum in double), so they decide nothing about contraction in the bodies that call them.  They are
// force-inlined functions on array references and a struct with a member array: a lambda that captures a register array keeps it in scratch.
#pragma once
#include "arl_util.h"

namespace strm {

constexpr int kThreads = 256;                // workgroup size of every stream kernel
typedef float f32x4v __attribute__((ext_vector_type(4)));

template <int D> inline constexpr int kLD = D + 4;                       // row stride of a stage in LDS, in floats
template <int D> inline constexpr int kStageFloats = 64 * kLD<D>;        // one LDS buffer

// br = the lane's quarter of resident row r (zero past nR)
template <int D>
__device__ __forceinline__ void load_resident(const float *Xr, int r, int nR, int g, float (&br)[D / 4]) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int i = 0; i < Q; i += 4) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < nR) v = *reinterpret_cast<const float4 *>(Xr + (size_t)r * D + Q * g + i);
        br[i] = v.x; br[i + 1] = v.y; br[i + 2] = v.z; br[i + 3] = v.w;
    }
}

// One stage in flight: 64 x D floats = 16 D float4s over 256 threads.  fetch() reads the 64 rows from t0 on (clamped to nT - 1: the caller masks
// rows past its end), stash() puts them into an LDS buffer.
template <int D>
struct stage {
    static constexpr int Q = D / 4, PF = 64 * Q / kThreads, FSTEP = kThreads / Q;
    f32x4v pre[PF];
    const int frow, fq;                      // this thread's row (+ i * FSTEP) and column of a stage
    __device__ __forceinline__ explicit stage(int tid) : frow(tid / Q), fq((tid % Q) * 4) {}
    __device__ __forceinline__ void fetch(const float *Xt, int t0, int nT) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int t = min(t0 + frow + i * FSTEP, nT - 1);
            pre[i] = *reinterpret_cast<const f32x4v *>(Xt + (size_t)t * D + fq);
        }
    }
    __device__ __forceinline__ void stash(float *tile_buf) const {
#pragma unroll
        for (int i = 0; i < PF; ++i) *reinterpret_cast<f32x4v *>(&tile_buf[(frow + i * FSTEP) * kLD<D> + fq]) = pre[i];
    }
};

// where lane (c, g) reads its A operand of tile `sub` of a staged buffer
template <int D>
__device__ __forceinline__ const float *a_row(const float *T, int sub, int c, int g) { return T + (sub * 16 + c) * kLD<D> + (D / 4) * g; }

// THE score sequence: the 16 x 16 tile of the rows whose quarters the lanes point at (LDS or global memory) against the resident rows, k ascending.
// The matrix core computes each element as its own k-ordered chain, so a pair's score has the same bits wherever this sequence produced it.
template <int D>
__device__ __forceinline__ f32x4v scores(const float *arow, const float (&br)[D / 4]) {
    f32x4v sc = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < D / 4; i += 4) {
        const float4 a = *reinterpret_cast<const float4 *>(arow + i);
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, br[i], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, br[i + 1], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, br[i + 2], sc, 0, 0, 0);
        sc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, br[i + 3], sc, 0, 0, 0);
    }
    return sc;
}

// the same sequence for four tiles at once on four independent accumulators (the 16x16x4 form needs >= 2 to reach its issue rate)
template <int D>
__device__ __forceinline__ void scores4(const float *a0, const float *a1, const float *a2, const float *a3, const float (&br)[D / 4], f32x4v (&sc)[4]) {
#pragma unroll
    for (int sub = 0; sub < 4; ++sub) sc[sub] = f32x4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < D / 4; i += 4) {
        const float4 a[4] = {*reinterpret_cast<const float4 *>(a0 + i), *reinterpret_cast<const float4 *>(a1 + i), *reinterpret_cast<const float4 *>(a2 + i),
                             *reinterpret_cast<const float4 *>(a3 + i)};
#pragma unroll
        for (int sub = 0; sub < 4; ++sub) {
            sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].x, br[i], sc[sub], 0, 0, 0);
            sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].y, br[i + 1], sc[sub], 0, 0, 0);
            sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].z, br[i + 2], sc[sub], 0, 0, 0);
            sc[sub] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[sub].w, br[i + 3], sc[sub], 0, 0, 0);
        }
    }
}
// the four tiles of a staged buffer
template <int D>
__device__ __forceinline__ void scores4(const float *T, int c, int g, const float (&br)[D / 4], f32x4v (&sc)[4]) {
    const float *a = a_row<D>(T, 0, c, g);
    scores4<D>(a, a + 16 * kLD<D>, a + 32 * kLD<D>, a + 48 * kLD<D>, br, sc);
}

// the second product: o[r = 4 g + reg][16 n + c] += sum_j pj[j] T[16 sub + 4 g + j][16 n + c], pj = the weights of tile `sub` as scores() left them
template <int D>
__device__ __forceinline__ void accumulate(const float *T, int sub, int c, int g, const float (&pj)[4], f32x4v (&o)[D / 16]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float *brow = T + (sub * 16 + 4 * g + j) * kLD<D> + c;
#pragma unroll
        for (int n = 0; n < D / 16; ++n) o[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(pj[j], brow[16 * n], o[n], 0, 0, 0);
    }
}

// second level of the weighted row sums: a stage's 64 streamed rows are summed in fp32 on the matrix cores, the stages in double
template <int D>
__device__ __forceinline__ void flush_stage(f32x4v (&o)[D / 16], double (&o2)[D / 16][4]) {
#pragma unroll
    for (int n = 0; n < D / 16; ++n) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o2[n][reg] += (double)o[n][reg];
        o[n] = f32x4v{0.f, 0.f, 0.f, 0.f};
    }
}

// out [split][nR][D] <- the wave's 16 x D tile (fp32 registers or the double second level)
template <int D, class Tile>
__device__ __forceinline__ void store_partial(float *out, int split, int nR, int r0, int g, int c, const Tile &o) {
#pragma unroll
    for (int n = 0; n < D / 16; ++n)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = r0 + 4 * g + reg;
            if (r < nR) out[((size_t)split * nR + r) * D + 16 * n + c] = (float)o[n][reg];
        }
}

// two running (max, sum of exp(. - max)) states into one; symmetric in its two states bit for bit (contraction off)
__device__ __forceinline__ void merge_lse(float &m, float &s, float m2, float s2) {
#pragma clang fp contract(off)
    const float M = fmaxf(m, m2);
    const float e1 = m == M ? 1.f : expf(m - M), e2 = m2 == M ? 1.f : expf(m2 - M);
    const float p1 = s * e1, p2 = s2 * e2;
    s = p1 + p2;
    m = M;
}

// ---- host side.  The split count decides the summation order, hence the bits: one function per distinct rule.

inline bool shape_ok(int64_t n_a, int64_t n_b, int64_t d) {
    return arl_width_ok(d) && n_a > 0 && n_b > 0 && n_a <= 0x7fffffffll / 128 && n_b <= 0x7fffffffll / 128;
}

// splits of the streamed table when n_resident rows are resident: enough workgroups to fill the chip several times over, at least 4 096 streamed
// rows each; the caller streams ceil(n_streamed / splits) rows per split
inline int split_count(int64_t n_resident, int64_t n_streamed) {
    const int64_t row_blocks = (n_resident + 63) / 64;
    int64_t s = (2048 + row_blocks - 1) / row_blocks;
    const int64_t max_s = (n_streamed + 4095) / 4096;
    if (s > max_s) s = max_s;
    if (s > 256) s = 256;
    return (int)(s < 1 ? 1 : s);
}

// the same with at least 1 024 streamed rows each and splits of whole 64-row stages
struct split { int ns, len; };
inline split stage_splits(int64_t n_resident, int64_t n_streamed) {
    const int64_t blocks = (n_resident + 63) / 64;
    int64_t s = (2048 + blocks - 1) / blocks;
    const int64_t max_s = (n_streamed + 1023) / 1024;
    if (s > max_s) s = max_s;
    if (s > 256) s = 256;
    if (s < 1) s = 1;
    const int64_t len = ((n_streamed + s - 1) / s + 63) / 64 * 64;
    return split{(int)((n_streamed + len - 1) / len), (int)len};
}

}  // namespace strm

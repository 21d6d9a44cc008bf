/*
 * arlib_amd.h -- C ABI of libarlib_amd.so: the MI355X (gfx950) implementation of ARLib's
 * embedding-recommender training + white-box attack hot path.
 *
 * The reference (CoderWZW/ARLib) is 100 % Python and has no FFI: its "kernels" are implicit ATen ops.
 * Each entry point below therefore cites the reference Python lines whose device work it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - return 0 on success; negative = argument error (ARL_E_*); positive = hipError_t.
 *   - never throws across the ABI, never allocates or frees device memory, takes no ownership:
 *     every buffer and workspace is caller-allocated; sizes of workspaces come from *_workspace_bytes.
 *   - device entry points are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default
 *     stream) and re-entrant across distinct streams as long as workspaces are distinct.
 *   - all matrices are row-major fp32; all indices int32; row offsets int32 (nnz < 2^31).
 *   - "emb" tables are ONE contiguous [N,d] buffer: user rows first, item rows at row offset item_off.
 *   - d must be a multiple of 4 and <= 256 for the propagation kernels (reference default d = 64).
 */
#ifndef ARLIB_AMD_H
#define ARLIB_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARL_OK 0
#define ARL_E_NULL (-1)      /* required pointer is NULL                     */
#define ARL_E_DIM (-2)       /* unsupported embedding size / shape           */
#define ARL_E_RANGE (-3)     /* size out of the int32 index range            */
#define ARL_E_ARG (-4)       /* inconsistent arguments                       */

typedef void *arl_stream_t;

/* ABI version; bump on any signature change. */
int arl_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Host sampler -- replaces util/sampler.py:4-30 (next_batch_pairwise) bit-exactly, including the
 * CPython `random` MT19937 stream it consumes (util/tool.py:101-108 seedSet -> random.seed).
 * `mt_state` is random.getstate()[1] as 625 uint32 (624 words + index); it is advanced in place so
 * the caller can random.setstate() it back and stay in lock-step with the reference.
 * Not thread-safe per state object.
 * ---------------------------------------------------------------------------------------------- */
/* random.seed(int): key = 32-bit little-endian words of abs(seed) */
int arl_mt_seed(uint32_t *mt_state, const uint32_t *key, int64_t key_len);
/* util/sampler.py:9   shuffle(training_data) in place; pairs = int32 [nnz][2] (user id, item id) */
int arl_sampler_shuffle(uint32_t *mt_state, int32_t *pairs, int64_t nnz);
/* random.sample(range(n), k) of CPython 3.10 on the caller's MT19937 state -- what the graph augmentations of the
 * contrastive encoders draw (recommender/SGL.py:281-299: edge / node dropout).  use_pool: the caller evaluates CPython's
 * set-size rule (n <= 21 + (k > 5 ? 4 ** ceil(log(3k, 4)) : 0)).  scratch: n int32 (pool form) or (n+31)/32 int32. */
int arl_mt_sample_range(uint32_t *mt_state, int64_t n, int64_t k, int32_t use_pool, int32_t *out, int32_t *scratch);
/* attack/Gray/GOAT.py:105-135  one itemSample(k, O_u, O_g, O_i) call for n_fake fake users on the caller's MT19937 state.
 *   rowptr / items : the interaction matrix as CSR (ascending item ids per user);  int_num [n_items]: itemIntNum as doubles;
 *   targets [n_targets]: the target items (excluded from the fill draws);  min_items = O_u * n_items and thr = int(O_i * n_users), both
 *   evaluated by the caller as Python evaluates them.
 * realUser starts empty per CALL: the first fake row draws randint(0, n_users - 1) until a user with degree >= min_items comes (the caller
 * should make sure one exists, where the reference would never return: without one this returns ARL_E_ARG before it draws), every later row
 * keeps that user.  Its items are walked ascending into I_s
 * (int_num > thr, fewer than ks = int(0.3 k) so far) or else I_f (int_num > thr / 3.0, fewer than int(0.7 k)); I_s is filled to ks, then I_f
 * until both hold k, each by one random.sample(pool, m) over the ASCENDING remaining ids (range(n_items) minus targets, I_s, I_f): the
 * pool is not built, its r-th id is found by a search in the sorted excluded ids.  That is CPython's order of the set only while
 * k + n_targets <= 0.4 * n_items (else ARL_E_RANGE: the caller evaluates the reference's expression in Python).
 *   out_s [n_fake][ks], out_f [n_fake][k - ks], out_real [n_fake][k] (1 where the candidate is an item of the real user), out_user [1];
 *   scratch: arl_goat_item_sample_scratch_words(n_items, k, n_targets) int32 words, no initialisation needed. */
int64_t arl_goat_item_sample_scratch_words(int64_t n_items, int64_t k, int64_t n_targets);
int arl_goat_item_sample(uint32_t *mt_state, const int64_t *rowptr, const int32_t *items, int64_t n_users, int64_t n_items,
                         const double *int_num, const int32_t *targets, int64_t n_targets, int64_t n_fake, int64_t k, double min_items,
                         int64_t thr, int32_t *out_s, int32_t *out_f, uint8_t *out_real, int32_t *out_user, int32_t *scratch);
/* util/sampler.py:12-29  one batch: positives pairs[begin..begin+count), one negative per positive drawn
 * by choice(item_list) with rejection against training_set_u[user] (given as a CSR with sorted item
 * ids; users >= memb_rows have an empty set, which is what the reference's defaultdict gives users
 * injected after DataLoader construction). */
int arl_sampler_next_batch(uint32_t *mt_state, const int32_t *pairs, int64_t begin, int64_t count,
                           int32_t n_items, const int64_t *memb_rowptr, const int32_t *memb_items,
                           int64_t memb_rows, int32_t *out_u, int32_t *out_p, int32_t *out_n);

/* ------------------------------------------------------------------------------------------------
 * CSR adjacency + long-row plan.  The plan splits rows longer than `chunk` edges into chunk tasks so
 * a 100k-edge popular-item row does not serialise one wavefront; partial sums go to `partial`
 * ([n_chunks][d] fp32, caller-allocated) and are combined in chunk order (deterministic).
 * n_chunks == 0 means "no plan": every row is processed whole.
 * ---------------------------------------------------------------------------------------------- */
typedef struct arl_csr {
    int64_t n_rows;
    int64_t nnz;
    const int32_t *rowptr;      /* [n_rows+1] device */
    const int32_t *col;         /* [nnz] device      */
    const float *val;           /* [nnz] device      */
    int32_t chunk;              /* rows with more than `chunk` edges are split (0 = never)       */
    int64_t n_chunks;
    const int32_t *chunk_row;   /* [n_chunks] device: output row of the task                      */
    const int32_t *chunk_begin; /* [n_chunks] device: first edge                                  */
    const int32_t *chunk_end;   /* [n_chunks] device: one past last edge                          */
    int64_t n_long;
    const int32_t *long_row;    /* [n_long] device                                                */
    const int32_t *long_first;  /* [n_long] device: first chunk slot of the row                   */
    const int32_t *long_count;  /* [n_long] device: number of chunk slots                         */
    float *partial;             /* [n_chunks * d] device workspace                                */
    const int32_t *row_tasks;   /* optional [n_rows][4] = (row, first edge, one past last edge, 0): the rows in the order the flag-masked
                                 * hop should take them -- sorted by edge count, so that the four lane groups of a wave own rows of equal
                                 * length (a wave lasts as long as its longest row).  NULL: rows in index order.               */
} arl_csr;

/* Degree-normalised edge values on device.  Replaces util/DataLoader.py:73-87 (normalize_graph_mat) and
 * recommender/LightGCN.py:212-215 (_init_uiAdj): val[e] = (dinv[row]*w[e])*dinv[col[e]], dinv = rowsum^-1/2
 * (0 for an empty row).  dinv: [n_rows] device workspace (kept: PGA re-uses it, attack/White/PGA.py:118-126). */
int arl_norm_adj_values_f32(int64_t n_rows, const int32_t *rowptr, const int32_t *col, const float *w,
                            float *dinv, float *val, arl_stream_t stream);
/* Same result for callers that keep the row id of every edge (erow[e], CSR order): the edge values are computed edge-parallel
 * (no wave per row).  All arrays 16-byte aligned. */
int arl_norm_adj_values_coo_f32(int64_t n_rows, const int32_t *rowptr, const int32_t *erow, const int32_t *col,
                                const float *w, int64_t nnz, float *dinv, float *val, arl_stream_t stream);
/* The value pass alone, for a caller that already has dinv (PGA: the row sums of its fixed-pattern graph follow from the F x I fake
 * block in O(F I), so the 77 M-edge row-sum pass is not needed): val[e] = (dinv[erow[e]] * w[e]) * dinv[col[e]]. */
int arl_norm_vals_coo_f32(const int32_t *erow, const int32_t *col, const float *w, int64_t nnz, const float *dinv, float *val,
                          arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SpMM family -- replaces torch.sparse.mm(sparse_norm_adj, ego) and its autograd
 * (recommender/LightGCN.py:234, recommender/SimGCL.py:202) plus the fused neighbours:
 *   arl_spmm_csr_f32          Y = alpha*(A X) + beta*Z            (Z may be NULL iff beta == 0)
 *   arl_spmm_csr_layersum_f32 Y = A X ; S = S_in + Y              (torch.stack(...).mean running sum,
 *                                                                  LightGCN.py:236-237; S may alias S_in)
 *   arl_spmm_csr_adam_f32     g = alpha*(A X) + beta*Z ; Adam(P,M,V; g)   (last backward hop fused with
 *                                                                  torch.optim.Adam.step, LightGCN.py:64)
 * X, Y, Z, S, P, M, V: [n_rows, d] (square adjacency).  Y must not alias X.
 * ---------------------------------------------------------------------------------------------- */
int arl_spmm_csr_f32(const arl_csr *A, const float *X, int64_t d, float alpha, float beta, const float *Z,
                     float *Y, arl_stream_t stream);
int arl_spmm_csr_layersum_f32(const arl_csr *A, const float *X, int64_t d, const float *S_in, float *S,
                              float *Y, arl_stream_t stream);
int arl_spmm_csr_adam_f32(const arl_csr *A, const float *X, int64_t d, float alpha, float beta, const float *Z,
                          const uint8_t *zflags, float *P, float *M, float *V, float lr, float beta1, float beta2,
                          float eps, int64_t step, arl_stream_t stream);

/* Sparse-batch-gradient forms.  In one training step dL/d(out) (= G) is non-zero on at most 3B rows and the last forward
 * hop is consumed on those rows only, so two of the 2L full-graph hops of recommender/LightGCN.py:230-240 + autograd
 * collapse to work proportional to the batch neighbourhood (results identical to the dense hops):
 *   arl_spmm_csr_flagged_f32  Y = alpha*(A X) + beta*Z where X is zero except on rows whose bit is set in the bitmap xbits
 *                             (uint32 words, bit c&31 of word c>>5; NULL = dense gather) and Z is read only where
 *                             zflags != 0 (NULL = everywhere).  xbits: ceil(n_cols/32) words, zflags: [n_rows] bytes.
 *   arl_spmm_csr_rows_f32     out_c[t] = alpha * w[t] * ( sum_k layers[k][rows[t]] + (A X)[rows[t]] ), t < n_rows_sel: only the
 *                             listed rows are produced (duplicates allowed).  A row of len edges is cut into max(1, ceil(len / P))
 *                             pieces, P = 1024 edges, doubled on the device until all pieces fit the workspace: `nsplit` is its
 *                             capacity in pieces per listed row on average, workspace =
 *                             arl_spmm_csr_rows_workspace_bytes(n_rows_sel, nsplit, d) (nsplit = 1, a workspace too small for
 *                             the piece tables, or more than 8192 listed rows -- the piece tables are built by one workgroup --:
 *                             every row cut into nsplit equal ranges).  The result is a deterministic function
 *                             of (graph, rows, nsplit).  layers: HOST array of
 *                             n_layers (<= 8) device pointers to [n_rows, d] tables.  row_weight: optional [n_rows_sel] factors
 *                             w (NULL = 1; the user-sharded step passes 1 for samples whose user the rank owns, 0 otherwise).
 *   arl_spmm_csr_rows_pieces_f32   the same with the starting P given (piece_edges; 0 = the default): tuning sweeps.
 *   arl_spmm_csr_rows_scratch_offset   index (in 32-bit words) of the pair {P used, piece count} that the call leaves in the
 *                             workspace, followed by the n_rows_sel + 1 piece offsets of the listed rows; -1 = equal-range form.
 *   arl_spmm_csr_adam_f32's zflags has the same meaning (NULL = read Z everywhere).
 *   arl_mark_rows_u8 / arl_zero_rows_f32: flags[idx[t]] = value / dst[idx[t], :] = 0 -- set and clear the batch's sparse state. */
int arl_spmm_csr_flagged_f32(const arl_csr *A, const float *X, int64_t d, const uint32_t *xbits, float alpha, float beta,
                             const float *Z, const uint8_t *zflags, float *Y, arl_stream_t stream);
int64_t arl_spmm_csr_rows_workspace_bytes(int64_t n_rows_sel, int64_t nsplit, int64_t d);
int arl_spmm_csr_rows_f32(const arl_csr *A, const float *X, int64_t d, const int32_t *rows, int64_t n_rows_sel,
                          int64_t nsplit, const float *const *layers, int64_t n_layers, float alpha, const float *row_weight,
                          float *out_c, void *workspace, arl_stream_t stream);
int arl_spmm_csr_rows_pieces_f32(const arl_csr *A, const float *X, int64_t d, const int32_t *rows, int64_t n_rows_sel,
                                 int64_t nsplit, int64_t piece_edges, const float *const *layers, int64_t n_layers, float alpha,
                                 const float *row_weight, float *out_c, void *workspace, arl_stream_t stream);
int64_t arl_spmm_csr_rows_scratch_offset(int64_t n_rows_sel, int64_t nsplit, int64_t d);
int arl_mark_rows_u8(uint8_t *flags, const int32_t *idx, int64_t n, int32_t value, arl_stream_t stream);
/* set (set != 0) or clear the bits idx[t] of a bitmap with atomic OR / AND (duplicates allowed) */
int arl_mark_rows_bits_u32(uint32_t *bits, const int32_t *idx, int64_t n, int32_t set, arl_stream_t stream);
int arl_zero_rows_f32(float *dst, const int32_t *idx, int64_t n, int64_t d, arl_stream_t stream);
/* The three per-batch updates of the sparse-batch step on one index list, fused: G[idx[t]] += scale * row_scale[t] * src[t]
 * (row_scale optional, NULL = 1), flags[idx[t]] = 1, bit idx[t] of `bits` set -- and the clearing counterpart (rows zeroed, flag and
 * bit cleared).  Duplicates accumulate IN INDEX ORDER, one wave per distinct row, starting from the value already in G: the association
 * of CPU index_put_(accumulate=True), i.e. of the reference's gathers under autograd (recommender/LightGCN.py:51-56); no float atomics,
 * bit-identical from run to run.
 * dup_bits (optional, a second bitmap of the size of `bits`, all-zero on entry like `bits`): a first launch records in it the rows the list
 * names more than once, so that only those are summed by the ordered scan and every other row is a plain add (44 -> ~10 us at cfg2); the
 * clearing call takes the same pointer and zeroes it again.
 * An entry with row_scale[t] == 0 is ABSENT: nothing is added, its row is neither flagged nor marked nor counted as a duplicate (the user-sharded
 * step gives foreign samples factor 0 on a clamped row to keep static shapes: they must not pile up on that row). */
int arl_batch_rows_set_f32(float *G, uint8_t *flags, uint32_t *bits, const int32_t *idx, int64_t n, int64_t d,
                           const float *src, float scale, const float *row_scale, uint32_t *dup_bits, arl_stream_t stream);
int arl_batch_rows_clear_f32(float *G, uint8_t *flags, uint32_t *bits, const int32_t *idx, int64_t n, int64_t d,
                             uint32_t *dup_bits, arl_stream_t stream);

/* Register-blocked SpMM (d = 64: one column per lane; d = 128: two adjacent columns per lane, 16 operand rows in flight): the same three operations as arl_spmm_csr_f32 / _layersum_f32 / _adam_f32, for the rows
 * of a PLAN.  A wave owns up to rows_per_wave (16 or 32) output rows with register accumulators and consumes one record stream
 * sorted by (column block, row slot); waves carry equal edge counts (arl_lpt_deal) and are all resident, so they sweep X in step
 * and share the gathered rows through the L2.  Rows absent from the plan (longer than its hub threshold) are not written: the
 * caller runs them through the chunked CSR kernel.  Plans are built by arlib_amd/ops.py:BlockedPlan.
 * Summation order differs from the CSR kernel: results agree to fp32 rounding, not bitwise; each is deterministic. */
typedef struct arl_blocked {
    int64_t n_waves, rows_per_wave;
    int64_t loads_in_flight;    /* 16 or 32 operand rows requested per wave before the first is consumed            */
    const int32_t *wave_ptr;    /* [n_waves + 1] record offsets, multiples of 64                          */
    const int32_t *wave_rows;   /* [n_waves][rows_per_wave] output row id, -1 = unused slot               */
    const int32_t *rec_col;     /* column | slot << 24 (columns < 2^24); padding records have val 0       */
    const float *rec_val;
    /* split rows: a row longer than the plan's hub threshold is dealt as several PIECES (piece p of P takes every P-th edge of the
     * column-sorted row, so each piece sweeps the whole column range like an ordinary row); a piece's slot holds -(2 + t) in
     * wave_rows and its raw sum goes to partial[t]; after the sweep the n_split rows are combined in piece order (deterministic)
     * and run the epilogue.  n_split = 0: no split rows (partial and the split_* arrays may be NULL). */
    int64_t n_split;
    const int32_t *split_row;   /* [n_split] output row                                                    */
    const int32_t *split_first; /* [n_split] first piece                                                   */
    const int32_t *split_count; /* [n_split] number of pieces                                              */
    float *partial;             /* [n_pieces][64] workspace (d = 128 runs as two 64-column passes)         */
    int64_t waves_per_group;    /* 1, 2 or 4 wavefronts per workgroup (0 = 4): the dispatcher balances workgroups, not waves, over
                                 * the CUs, so a launch of ~12 waves per CU is spread evenly only with small workgroups         */
} arl_blocked;
int arl_spmm_blocked_f32(const arl_blocked *P, const float *X, int64_t d, float alpha, float beta, const float *Z,
                         const uint8_t *zflags, float *Y, arl_stream_t stream);
/* The flag-masked hop (arl_spmm_csr_flagged_f32) on the blocked plan: X is zero except on rows whose bit is set in xbits (required).  Each
 * lane tests the bit of its own record, a ballot gives the 64-record batch's hits and only those are gathered, in record order, so the result
 * has the bits of arl_spmm_blocked_f32 on the same operand.  The plan's hub rows stay with arl_spmm_csr_flagged_f32. */
int arl_spmm_blocked_flagged_f32(const arl_blocked *P, const float *X, int64_t d, const uint32_t *xbits, float alpha, float beta,
                                 const float *Z, const uint8_t *zflags, float *Y, arl_stream_t stream);
/* Y = alpha * diag(row_scale) (A X) + beta * Z: the product with a diagonal factor in the epilogue (PGA applies D^-1/2 W D^-1/2 in
 * factors and keeps W's values fixed); CSR and blocked schedules. */
int arl_spmm_csr_rscale_f32(const arl_csr *A, const float *X, int64_t d, const float *row_scale, float alpha, float beta,
                            const float *Z, float *Y, arl_stream_t stream);
int arl_spmm_blocked_rscale_f32(const arl_blocked *P, const float *X, int64_t d, const float *row_scale, float alpha,
                                float beta, const float *Z, float *Y, arl_stream_t stream);
int arl_spmm_blocked_layersum_f32(const arl_blocked *P, const float *X, int64_t d, const float *S_in, float *S, float *Y,
                                  arl_stream_t stream);
int arl_spmm_blocked_adam_f32(const arl_blocked *P, const float *X, int64_t d, float alpha, float beta, const float *Z,
                              const uint8_t *zflags, float *Pm, float *M, float *V, float lr, float beta1, float beta2,
                              float eps, int64_t step, arl_stream_t stream);
/* The same hops over the row sets [first, n_sets) of a WHOLE plan in one call (first > 0: the caller does not read the output rows of the
 * sets before it).  The sets' launches are followed by ONE combine of the split rows of all of them, and the masked hop runs the sets in one
 * grid where they agree on rows_per_wave (at most 4 sets; else one launch per set as above).  Every wave runs the records it runs in the
 * per-set calls and a split row adds the same pieces in the same order: the results have the bits of the per-set calls.
 * arl_blocked_hop is what the plan holds for that: the sets' split_row / split_first / split_count tables back to back in set order, with
 * split_first counting pieces of ONE workspace `partial` of which set k's own `partial` is the slice that starts at its first piece (64
 * floats per piece), and stream_len (HOST array, [n_sets], may be NULL = array order): records per wave of every set -- the merged masked grid
 * starts the set with the longest streams first.  hop may be NULL when no set that runs has split rows. */
typedef struct arl_blocked_hop {
    int64_t n_split;
    const int32_t *split_row, *split_first, *split_count;
    float *partial;
    const int64_t *stream_len;
} arl_blocked_hop;
int arl_spmm_blocked_sets_f32(const arl_blocked *sets, int64_t n_sets, int64_t first, const arl_blocked_hop *hop, const float *X, int64_t d,
                              float alpha, float beta, const float *Z, const uint8_t *zflags, float *Y, arl_stream_t stream);
int arl_spmm_blocked_flagged_sets_f32(const arl_blocked *sets, int64_t n_sets, int64_t first, const arl_blocked_hop *hop, const float *X,
                                      int64_t d, const uint32_t *xbits, float alpha, float beta, const float *Z, const uint8_t *zflags,
                                      float *Y, arl_stream_t stream);
int arl_spmm_blocked_rscale_sets_f32(const arl_blocked *sets, int64_t n_sets, int64_t first, const arl_blocked_hop *hop, const float *X,
                                     int64_t d, const float *row_scale, float alpha, float beta, const float *Z, float *Y,
                                     arl_stream_t stream);
int arl_spmm_blocked_layersum_sets_f32(const arl_blocked *sets, int64_t n_sets, int64_t first, const arl_blocked_hop *hop, const float *X,
                                       int64_t d, const float *S_in, float *S, float *Y, arl_stream_t stream);
int arl_spmm_blocked_adam_sets_f32(const arl_blocked *sets, int64_t n_sets, int64_t first, const arl_blocked_hop *hop, const float *X,
                                   int64_t d, float alpha, float beta, const float *Z, const uint8_t *zflags, float *Pm, float *M, float *V,
                                   float lr, float beta1, float beta2, float eps, int64_t step, arl_stream_t stream);
/* Host helper of the plan: rows sorted by edge count (descending) are dealt to the least loaded of n_bins waves with a free
 * slot (cap slots each); bin_out / slot_out receive the placement. */
int arl_lpt_deal(int64_t n, const int32_t *weight_desc, int64_t n_bins, int64_t cap, int32_t *bin_out, int32_t *slot_out);

/* SYN-v1, the benchmark's synthetic interaction graphs (no reference counterpart: ARLib ships fixed datasets, data/clean/),
 * generated natively.  Every random number is a counter-based hash h(stream, index) = splitmix64(splitmix64(seed ^ stream * PHI) ^ index):
 * log-normal user degrees (streams 1, 2), item draws with popularity density ~ x^-1/2 through a hash-derived item permutation (streams 3, 4),
 * one extra edge per item so that none is isolated (stream 5); user-major sorted, de-duplicated int32 (user, item) pairs.  Returns the pair
 * count; writes nothing and returns the count needed when pairs_out is NULL or capacity is too small.  arl_graph_digest is the
 * order-sensitive checksum both this generator and the numpy one (arlib_amd/util/synthetic.py) are compared by. */
int64_t arl_syn_v1_pairs(int64_t n_users, int64_t n_items, double mean_deg, uint64_t seed, double sigma, int64_t deg_min, int64_t deg_max,
                         int32_t *pairs_out, int64_t capacity);
uint64_t arl_graph_digest(const int32_t *pairs, int64_t n);

/* ------------------------------------------------------------------------------------------------
 * BPR + un-squared L2 on gathered rows, forward + backward in one call.
 * Replaces util/loss.py:5-9 (bpr_loss, eps 10e-8), :25-29 (l2_reg_loss), the three gathers
 * rec_user_emb[user_idx] ... (recommender/LightGCN.py:51-52) and their autograd (index_put accumulate).
 *   loss_out[0] = mean(-log(1e-7 + sigmoid(<u,p>-<u,n>)))   loss_out[1] = reg*(||U_b||_F + ||P_b||_F)
 *   loss_out[2] = ||U_b||_F   loss_out[3] = ||P_b||_F
 *   G[row] += upstream * d(loss)/d(emb[row]): duplicates accumulate IN SAMPLE ORDER (a user row: its samples' terms in order; an item
 *   row: its positive-role terms in order, then its negative-role ones -- autograd's three index_put_(accumulate) of the reference),
 *   one wave per distinct row, no float atomics, bit-identical from run to run; G pre-zeroed or holding other gradient terms.
 *   G may be NULL for forward only.  distinct_rows != 0: the caller guarantees that the 3B rows u[b], item_off + p[b], item_off + n[b]
 *   are pairwise distinct (the compact [3B, d] batch form) -- the ownership scan is skipped.
 * workspace: arl_bpr_l2_workspace_bytes(B) bytes of device memory.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_bpr_l2_workspace_bytes(int64_t B);
int arl_bpr_l2_fwd_bwd_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p,
                           const int32_t *n, int64_t B, float reg, float upstream, float *loss_out, float *G,
                           void *workspace, int32_t distinct_rows, arl_stream_t stream);

/* User-sharded form of the same loss (one process per GPU holds a block of users): the batch is split by
 * user shard, so the mean (1/B_global) and the two Frobenius norms need the whole batch.
 *   arl_bpr_l2_partial_f32  : per-sample coefficients into `workspace`, and sums_out[0..2] = sum of -log(...) terms,
 *                             sum |u|^2, sum |p|^2 over the B_local samples -> caller all-reduces (RCCL) the 3 floats.
 *   arl_bpr_l2_backward_f32 : scatter-adds the gradient of the B_local samples into G using norms4[2] = ||U_b||_F and
 *                             norms4[3] = ||P_b||_F of the WHOLE batch (same layout as loss_out above). */
int arl_bpr_l2_partial_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p,
                           const int32_t *n, int64_t B_local, int64_t B_global, float *sums_out, void *workspace,
                           arl_stream_t stream);
int arl_bpr_l2_backward_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p,
                            const int32_t *n, int64_t B_local, float reg, float upstream, const float *norms4, float *G,
                            const void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dense optimisers -- torch.optim.Adam (betas, eps, no weight decay; recommender/LightGCN.py:33,64) and
 * torch.optim.SGD (attack/White/PGA.py:59) over a whole table.  `step` is the 1-based step count.
 * ---------------------------------------------------------------------------------------------- */
int arl_adam_dense_f32(float *p, const float *g, float *m, float *v, int64_t n, float lr, float beta1,
                       float beta2, float eps, int64_t step, arl_stream_t stream);
int arl_sgd_dense_f32(float *p, const float *g, int64_t n, float lr, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Row gather / scatter-add helpers (advanced indexing of the propagated tables and its backward).
 *   gather:       dst[t] = src[idx[t]]
 *   scatter_add:  dst[idx[t]] += scale * src[t]   (duplicates accumulate in index order -- torch's CPU index_put_(accumulate=True)
 *                 association, the backward of the reference's advanced-index gathers; ordered, no float atomics, deterministic)
 *   axpy_unique:  dst[r] += alpha * src[r] once for every DISTINCT row r in idx (src, dst: tables of the same shape); dup_bits: optional bitmap
 *                 (as filled by arl_batch_rows_set_f32 for a list containing idx) of the rows that may be named twice -- the others skip the scan
 *   shard_batch_prep: user-sharded batch bookkeeping in one launch -- lu[b] = clamp(u[b] - u0, 0, Ul - 1), own [3B] = [(u0 <= u[b] < u1) | 1 | 1]
 *                 (factors of the batch's user / positive / negative contributions), item_rows = [p | n], rows_l = [lu | Ul + p | Ul + n] with Ul = u1 - u0 (no reference counterpart: main.py:19 pins one device)
 * ---------------------------------------------------------------------------------------------- */
int arl_gather_rows_f32(const float *src, const int32_t *idx, int64_t n, int64_t d, float *dst, arl_stream_t stream);
int arl_scatter_add_rows_f32(float *dst, const int32_t *idx, int64_t n, int64_t d, const float *src, float scale,
                             arl_stream_t stream);
int arl_rows_axpy_unique_f32(float *dst, const float *src, const int32_t *idx, int64_t n, int64_t d, float alpha,
                             const uint32_t *dup_bits, arl_stream_t stream);
int arl_shard_batch_prep_i32(const int32_t *u, const int32_t *p, const int32_t *n, int64_t B, int64_t u0, int64_t u1,
                             int32_t *lu, float *own, int32_t *item_rows, int32_t *rows_l, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * InfoNCE forward + backward -- replaces util/loss.py:42-49 and its autograd.
 *   loss_out[0] = mean_i( -log( exp(<a_i,b_i>/tau) / sum_j exp(<a_i,b_j>/tau) ) ), a,b = row-normalised v1,v2
 *   dv1, dv2 = upstream * gradients (may be NULL for forward only).   n <= 8192, d <= 256.
 * workspace: arl_infonce_workspace_bytes(n, d).
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_infonce_workspace_bytes(int64_t n, int64_t d);
int arl_infonce_fwd_bwd_f32(const float *v1, const float *v2, int64_t n, int64_t d, float tau, float upstream,
                            float *loss_out, float *dv1, float *dv2, void *workspace, arl_stream_t stream);

/* SimGCL perturbation -- recommender/SimGCL.py:203-205: E += sign(E) * normalize(noise, dim=-1) * eps, in place. */
int arl_simgcl_perturb_f32(float *E, const float *noise, int64_t n, int64_t d, float eps, arl_stream_t stream);
/* The same perturbation with the noise drawn inside the kernel (recommender/SimGCL.py:203-205: random_noise = torch.rand_like(ego)):
 *   dst[r, k] = src[r, k] + sign(src[r, k]) * u[r, k] / max(||u[r, :]||, 1e-12) * eps,
 *   u[r, k] = uniform [0, 1) from a counter-based hash of (seed, stream_id, row * d + k), row = row_ids ? row_ids[r] : r.
 * No noise table, no clone of the operand (dst may alias src); with row_ids the operand is a compact slice of a larger table and receives
 * exactly the noise its rows get in a full-table call with the same (seed, stream_id).  d <= 256. */
int arl_simgcl_perturb_rng_f32(const float *src, float *dst, int64_t n, int64_t d, const int32_t *row_ids, float eps, uint64_t seed,
                               uint64_t stream_id, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * NGCF layer glue -- recommender/NGCF.py:200-208:  E' = leaky_relu((P + E) W1 + (P * E) W2),  P = A_hat E.
 * The d x d products are ONE GEMM of [S | T] (N x 2d) with [W1; W2] (the caller's BLAS); these are the passes around it.
 *   combine      : ST[row] = [ P[row] + E[row] | P[row] * E[row] ]                       (ST: [n, 2d])
 *   act          : Z <- leaky_relu(Z, slope) in place;  acc += Z when acc != NULL        (layer sum)
 *   act_bwd      : gZ = gOut * (Out > 0 ? 1 : slope)
 *   combine_bwd  : from gST = [gS | gT]:  gP = gS + gT * E,  gE = gS + gT * P
 * d % 4 == 0.
 * ---------------------------------------------------------------------------------------------- */
int arl_ngcf_combine_f32(const float *P, const float *E, int64_t n, int64_t d, float *ST, arl_stream_t stream);
int arl_ngcf_act_f32(float *Z, float *acc, int64_t n, int64_t d, float slope, arl_stream_t stream);
int arl_ngcf_act_bwd_f32(const float *gOut, const float *Out, int64_t n, int64_t d, float slope, float *gZ, arl_stream_t stream);
int arl_ngcf_combine_bwd_f32(const float *gST, const float *P, const float *E, int64_t n, int64_t d, float *gP, float *gE,
                             arl_stream_t stream);
/* The same layer with its dense part on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulation; d in {16, 32, 64, 128}):
 * the [N, 2d] operand [P + E | P * E] of recommender/NGCF.py:200-208 is formed in registers, never in memory.
 *   fwd   : out = leaky_relu((P + E) W1 + (P * E) W2),  W = [W1; W2] as [2d, d] row-major
 *   dgrad : gZ = gOut * act'(Out);  gP = gS + gT * E,  gE = gS + gT * P  with [gS | gT] = gZ W^T;  Wt = W^T as [d, 2d] row-major; gZ is an output (wgrad reads it)
 *   wgrad : gW [2d, d] = [P + E | P * E]^T gZ, per-workgroup partials in `workspace` (arl_ngcf_wgrad_workspace_bytes) summed in a fixed order */
int arl_ngcf_dense_fwd_f32(const float *P, const float *E, const float *W, int64_t n, int64_t d, float slope, float *out, arl_stream_t stream);
int arl_ngcf_dense_dgrad_f32(const float *gOut, const float *Out, const float *P, const float *E, const float *Wt, int64_t n, int64_t d, float slope,
                             float *gZ, float *gP, float *gE, arl_stream_t stream);
int64_t arl_ngcf_wgrad_workspace_bytes(int64_t n, int64_t d);
int arl_ngcf_dense_wgrad_f32(const float *P, const float *E, const float *gZ, int64_t n, int64_t d, float *gW, void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * NCF MLP tower -- replaces the tower loop and the two torch.cat of recommender/NCF.py:203-220
 *   (Linear(d, 5d) -> ReLU -> Linear(5d, 2d) -> ReLU -> Linear(2d, d) -> ReLU, nn.Linear weights [out, in] row-major, biases [out]).
 * One kernel, exact fp32 on v_mfma_f32_16x16x4_f32, the activations of a row tile kept in registers; d in {16, 32, 64, 128}.
 *   fwd : out[r] = [mf[s] | tower(mlp[s])] as [n, 2d], s = rows[r] (rows != NULL: rows form, entries may repeat) or s = r (rows == NULL:
 *         table form over the first n rows).  h1 [n, 5d] and h2 [n, 2d] (both or neither): the ReLU outputs backward needs.
 *   bwd : from g_out [n, 2d] (its tower half, columns d .. 2d, is read), out, h1, h2 of a rows-form call and the same mlp / rows / weights:
 *         g_mlp_rows [n, d] = the gradient of the tower's input rows (in row order; duplicates are NOT summed here), and
 *         g_params = [gW0 | gb0 | gW1 | gb1 | gW2 | gb2] (17 d^2 + 8 d floats, nn.Linear layouts) summed over the n rows.  ReLU gradient
 *         out > 0 (torch's threshold_backward).  The sums run over per-chunk partials (a fixed split of the rows that depends on n alone)
 *         folded in a fixed order: no float atomics, bit-identical from run to run.
 * workspace: arl_ncf_tower_bwd_workspace_bytes(n, d) bytes of device memory.
 * ---------------------------------------------------------------------------------------------- */
int arl_ncf_tower_fwd_f32(const float *mf, const float *mlp, const int32_t *rows, int64_t n, int64_t d, const float *W0, const float *b0,
                          const float *W1, const float *b1, const float *W2, const float *b2, float *out, float *h1, float *h2, arl_stream_t stream);
int64_t arl_ncf_tower_bwd_workspace_bytes(int64_t n, int64_t d);
int arl_ncf_tower_bwd_f32(const float *g_out, const float *out, const float *h1, const float *h2, const float *mlp, const int32_t *rows, int64_t n,
                          int64_t d, const float *W0, const float *W1, const float *W2, float *g_mlp_rows, float *g_params, void *workspace,
                          arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * WRMF loss + un-squared L2 on gathered rows, forward + backward in one call.
 * Replaces util/loss.py:11-15 (wrmf_loss), :25-29 (l2_reg_loss), the gathers of recommender/WRMF.py:40-43 and their autograd.
 *   loss_out[0] = SUM_b  pos_weight (<u,p> - 1)^2 + <u,n>^2   (a sum over the batch, as the reference; not a mean)
 *   loss_out[1] = reg*(||U_b||_F + ||P_b||_F)   loss_out[2] = ||U_b||_F   loss_out[3] = ||P_b||_F
 *   G[row] += upstream * d(loss)/d(emb[row]) with the row order, ownership scan and determinism of arl_bpr_l2_fwd_bwd_f32 (no float
 *   atomics, bit-identical from run to run); G may be NULL; distinct_rows as there.
 * workspace: arl_wrmf_l2_workspace_bytes(B) bytes of device memory.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_wrmf_l2_workspace_bytes(int64_t B);
int arl_wrmf_l2_fwd_bwd_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p, const int32_t *n, int64_t B,
                            float pos_weight, float reg, float upstream, float *loss_out, float *G, void *workspace, int32_t distinct_rows,
                            arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Adversarial BPR term of APR / AMF (He et al., SIGIR'18; no counterpart in the reference), forward + backward in one call
 * (csrc/arl_advpair.hip).  Positions t = b (user of sample b), B + b (positive), 2B + b (negative); a position's row is READ at
 * emb[u[b]] / emb[item_off + p[b]] / emb[item_off + n[b]]; its NODE is groups[t] (int32 [3B], >= 0), or with groups == NULL the
 * row id itself, or with groups == NULL and distinct_rows the position (a per-sample perturbation).
 *   Gamma_g = sum, in ascending t, of d bpr / d(row of position t) over the positions of node g (bpr = the mean of
 *             arl_bpr_l2_fwd_bwd_f32's loss_out[0]);   delta_g = eps * Gamma_g / sqrt(max(|Gamma_g|^2, 1e-12))
 *   loss_out[0] = adv = mean_b -log(10e-8 + sigmoid(<u', p'> - <u', n'>)) on rows x' = x + delta_node(x);  loss_out[1] = clean bpr
 *   G[row] += upstream * d adv / d emb[row] with delta held constant, duplicates in ascending t on top of what G holds (no float
 *             atomics, bit-identical from run to run); distinct_rows: the 3B read rows are pairwise distinct (plain store-add).
 *   G may be NULL (losses only); delta_out: NULL or [3B, d], the perturbation each position received.
 * 1 <= d <= 256 (else ARL_E_DIM) and 3B <= 16384 (else ARL_E_RANGE): Gamma must be complete before any delta exists, so the
 * ownership scan is one window.  workspace: arl_bpr_adv_workspace_bytes(B, d) bytes (0 = unsupported shape).
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_bpr_adv_workspace_bytes(int64_t B, int64_t d);
int arl_bpr_adv_fwd_bwd_f32(const float *emb, int64_t d, int64_t item_off, const int32_t *u, const int32_t *p, const int32_t *n, int64_t B,
                            const int32_t *groups, float eps, float upstream, float *loss_out, float *G, float *delta_out, void *workspace,
                            int32_t distinct_rows, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * White-box attack primitives.
 * ---------------------------------------------------------------------------------------------- */
/* ------------------------------------------------------------------------------------------------
 * CLeaR spectral-feature-augmentation L1 term -- replaces spectral_feature_augmentation(H, 1) + F.l1_loss(SFA, H)
 * and their autograd (attack/White/CLeaR.py:98-125) for H = the rows of X taken w[row] times each
 * (H = cat(Pu[users], Pi[pos], Pi[neg]) repeats table rows; it is never materialised).
 *   r = H^T H r0;  loss_out[0] = mean| H - H r r^T/|r|^2  -  H |  over numel_h = rows(H) * d elements;
 *   G[row] (= or +=, per `accumulate`) scale * d loss / d X[row]   (G may be NULL: loss only).
 * X: [n_rows, d] row-major, d <= 256; w: [n_rows] multiplicities (0 = row not in H); r0: [d].
 * workspace: arl_sfa_workspace_bytes(n_rows, d).  Deterministic (two-stage reductions, no atomics).
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_sfa_workspace_bytes(int64_t n_rows, int64_t d);
int arl_sfa_l1_fwd_bwd_f32(const float *X, const float *w, const float *r0, int64_t n_rows, int64_t d, int64_t numel_h,
                           float scale, int32_t accumulate, float *loss_out, float *G, void *workspace, arl_stream_t stream);
/* The same term cut at its two global reductions, for row sets partitioned over ranks (the user-sharded CLeaR surrogate step: the rows of H
 * generated by a rank's own users -- their rows, the targets with weight = local real users, the local negatives' histogram): the caller
 * sum-all-reduces r_out[d] after stage 1 and as_out[d + 1] = [a | S] after stage 2, then hands the reduced vectors to stage 3, which
 * writes loss_out (the GLOBAL loss when numel_h is the global element count) and this rank's rows of G.  One workspace for all stages
 * (arl_sfa_workspace_bytes).  stage1; stage2; stage3 without reductions = arl_sfa_l1_fwd_bwd_f32 (attack/White/CLeaR.py:98-125). */
int arl_sfa_stage1_f32(const float *X, const float *w, const float *r0, int64_t n_rows, int64_t d, float *r_out, void *workspace,
                       arl_stream_t stream);
int arl_sfa_stage2_f32(const float *X, const float *w, const float *r, int64_t n_rows, int64_t d, float *as_out, void *workspace,
                       arl_stream_t stream);
int arl_sfa_stage3_f32(const float *X, const float *w, const float *r0, const float *r, const float *as, int64_t n_rows, int64_t d,
                       int64_t numel_h, float scale, int32_t accumulate, float *loss_out, float *G, void *workspace, arl_stream_t stream);

/* Gradient w.r.t. adjacency values restricted to `rows`, dense over the item block (the only entries PGA
 * uses; replaces autograd.grad(Loss, sparse_norm_adj) + to_dense() + slicing, attack/White/PGA.py:117-134):
 *   out[t, j] += <dY[rows[t]], X[col_off + j]> ,  0 <= j < n_cols.   out: [n_rows_sel, n_cols]. */
int arl_sddmm_rows_dense_f32(const float *dY, const float *X, int64_t d, const int32_t *rows, int64_t n_rows_sel,
                             int64_t col_off, int64_t n_cols, float *out, arl_stream_t stream);
/* Gradient w.r.t. EVERY stored entry of the adjacency (CSR order): gval[e] += alpha * <dY[row(e)], X[col[e]]> -- the autograd of
 * torch.sparse.mm with respect to its sparse argument, as accumulated by train(requires_adjgrad=True) (recommender/LightGCN.py:41-43,58-59);
 * d % 4 == 0, d <= 256, 16-byte aligned tables.  One writer per entry (deterministic). */
int arl_sddmm_csr_f32(const int32_t *rowptr, const int32_t *col, int64_t n_rows, int64_t d, const float *dY, const float *X, float alpha,
                      float *gval, arl_stream_t stream);
/* out = alpha * (tables[0] + ... + tables[n_tables-1]), element-wise over n_elems floats (n_elems % 4 == 0, 1 <= n_tables <= 8): the mean
 * over the propagated layers (recommender/LightGCN.py:236-240: torch.stack(...).mean) in one pass.  tables: HOST array of device pointers;
 * out may alias one of them. */
int arl_tables_sum_f32(const float *const *tables, int64_t n_tables, int64_t n_elems, float alpha, float *out, arl_stream_t stream);

/* The F x I fake-user block S of the poisoned adjacency applied as two dense products (attack/White/PGA.py:118-134 multiplies by the
 * dense (U+F+I)^2 matrix; the factored operator needs only these two blocks of it).  S: [F, I] row-major, d % 4 == 0, d <= 256.
 *   rows:  Y[f, :] += alpha * rscale[f] * sum_i S[f, i] * X[i, :]      X: [I, d] (the item rows), Y: [F, d], rscale: [F] or NULL (= 1)
 *   cols:  Y[i, :] += alpha * rscale[i] * sum_f S[f, i] * Xf[f, :]     Xf: [F, d] (the fake users' rows), Y: [I, d], rscale: [I] or NULL
 * fp32 FMA chains in a fixed order (the row product is split over 64-item chunks whose partials are added in a fixed tree):
 * deterministic.  workspace (rows only): arl_fake_block_rows_workspace_bytes(F, I, d) bytes of device memory. */
int64_t arl_fake_block_rows_workspace_bytes(int64_t F, int64_t I, int64_t d);
int arl_fake_block_rows_f32(const float *S, int64_t F, int64_t I, const float *X, int64_t d, const float *rscale, float alpha, float *Y,
                            void *workspace, arl_stream_t stream);
int arl_fake_block_cols_f32(const float *S, int64_t F, int64_t I, const float *Xf, int64_t d, const float *rscale, float alpha, float *Y,
                            arl_stream_t stream);
/* Projected-gradient step on the fake-user block S [rows, cols] (attack/White/PGA.py:118-139):
 *   g = dinv_rows[r] * grad[r,c] * dinv_cols[c]   (D^-1/2 grad D^-1/2; either scale vector may be NULL = 1)
 *   g = 0 where S[r,c] == 0                       (autograd.grad on a sparse tensor only yields pattern entries)
 *   S = S - 0.2*tanh(g);  S > 1 -> 1;  S <= 0 -> 10e-8 */
int arl_pga_update_f32(float *S, const float *grad, const float *dinv_rows, const float *dinv_cols, int64_t rows,
                       int64_t cols, arl_stream_t stream);
/* Streaming scores + interacted mask + top-k, never materialising U x I.  Replaces the chunked Pu@Pi.T into a
 * host buffer, scores[nonzero] = -10e8 and torch.topk (attack/White/DLAttack.py:73-83, CLeaR.py:75-82,
 * PGA.py:100-102 with mask_rowptr == NULL).  Output sorted by descending score, ties by ascending item id.
 * k <= 128.
 * workspace == NULL: scores are the exact fp32 contraction (bitwise an fmaf chain over d).
 * workspace != NULL (arl_score_mask_topk_workspace_bytes(I, d) bytes) and d in {64, 128}: the contraction runs on
 * the 16-bit matrix path with every fp32 operand (scaled by a power of two chosen per table on the device) split in
 * two fp16 pieces, three partial products accumulated in fp32, 3x faster; the workspace receives the split image of Pi, the
 * two tables' largest magnitudes and their smallest nonzero row maxima.  Other d ignore the workspace.
 * Contract (either path): every returned pair has |top_val - float64 score| <= (d 2^-24 + 2^-21) |Pu row| |Pi row| (d 2^-24 alone with
 * workspace == NULL), and an item of the float64 list that is missing was displaced by a near-tie within that bound.  The split keeps it only
 * for rows that are not tiny next to their table (one scale per table): if a nonzero row's largest |element| is below 2^-16 of its table's, or
 * a table's largest magnitude has an exponent outside [-27, 53], the split builds return at once and the exact fp32 build writes the same
 * outputs -- decided on the device, no host wait.  All-zero rows do not count; non-finite tables are outside the contract.  (How the three products are scheduled is internal: the
 * stream contracts the high pieces only, filters against threshold - E with E a rigorous bound on the two other products,
 * and every candidate that reaches a list is scored with all three -- the scores returned are those of the three-product form.)
 * warm_idx (optional, matrix-core path only): [U, k] DISTINCT candidate items per user, e.g. the previous call's top_idx when
 * the tables moved little; it only pre-sets each user's threshold (same result, ~6x fewer list inserts).  If a candidate has
 * become masked the threshold may exclude too much: *underflow (int32, zeroed by the caller) is then set non-zero and the
 * same call repeats the pass cold -- a second launch that every workgroup leaves at once unless the flag is set, decided on
 * the device: top_idx / top_val are valid in stream order either way and the host never has to read the flag (it stays
 * readable as a statistic).
 * item_order (optional, used on the fp16 matrix path; a permutation of [0, I)): the items are STREAMED in this order instead of table
 * order -- typically by descending row norm, so that the items most users rank high come first and the thresholds rise early (6-20 %
 * less time at 1 M x 100 K).  Masks, warm_idx, top_idx and the tie order (lower item id first) are in item ids as always: the result is
 * the one of the table order, bit for bit.
 * Early exit (fp16 matrix path): with the stream in descending row-norm order a workgroup stops streaming once, for each of its users,
 * |a_u| * (largest norm of any later item) lies below the user's current k-th best score by more than the pre-filter's slack (Cauchy-Schwarz:
 * no later item can enter a list) -- the stages skipped cannot change the result, which stays that of the full stream bit for bit.  What was
 * skipped is readable after the pass: two uint64 counters at byte arl_score_mask_topk_stats_offset(I, d) of the workspace,
 * [stream stages consumed summed over workgroups, workgroups], followed by four int32 [exit build picked, plain build picked, split path taken,
 * exact fp32 fallback taken].
 * The exit's code costs the stream loop ~5 % where nothing can be skipped (the loop has no register to spare), so it lives in a second BUILD of
 * the kernel.  exit_mode = 1: both builds are launched and the device runs one of them, chosen from the items' norm profile (the exit build iff the
 * norms at 7/8 of the stream are below half of the 4096th largest); exit_mode = 0: the plain build alone (a caller that has seen the counters report
 * nothing skipped on these tables saves the 5 %).  Results are identical in every case.
 * user_workspace (optional; arl_score_mask_topk_user_workspace_bytes(U, d) bytes, 16-byte aligned like the workspace; fp16 matrix path, d = 64): selects the SECOND FORM of the stream --
 * a wave owns 32 users and contracts 32 x 32 tiles with the items as rows, so that all of a lane's scores belong to one user and the pre-filter is one
 * subtract + one bit shift per score; 512 users share a staged tile; the sorted lists are kept in top_idx / top_val themselves while the pass runs;
 * the starting thresholds (bootstrap sample, warm-start candidates) come from two small launches of their own.  The workspace receives the split
 * image of Pu and the starting thresholds.  Candidates, exact scores, keys and tie order are those of the first form: results identical bit for bit,
 * 1.6x less time at 1 M x 100 K.  NULL: the first form.  (exit_mode = 1 launches the second form's own two builds; the device picks as before.) */
int64_t arl_score_mask_topk_workspace_bytes(int64_t I, int64_t d);
int64_t arl_score_mask_topk_user_workspace_bytes(int64_t U, int64_t d);
int64_t arl_score_mask_topk_stats_offset(int64_t I, int64_t d);
int arl_score_mask_topk_f32(const float *Pu, const float *Pi, int64_t U, int64_t I, int64_t d,
                            const int32_t *mask_rowptr, const int32_t *mask_col, int64_t k, int32_t *top_idx,
                            float *top_val, void *workspace, const int32_t *warm_idx, int32_t *underflow,
                            const int32_t *item_order, int32_t exit_mode, void *user_workspace, arl_stream_t stream);
/* CW term of the white-box attacks' surrogate loss, from the users' top-k lists (attack/White/CLeaR.py:83-95, PGA.py:104-116; the reference builds
 * three Python lists of U*T ids and gathers a [U*T, d] matrix per side).  X [n_user_rows + n_items, d] = the packed propagated tables (users first);
 * pairs = (real user u < n_real) x (target t): negative item neg(u, t) = top_idx[u][k - 1 - t] (the successive .pop()s of CLeaR.py:84-88), positive
 * = targets[t] (item ids, int64, on the device).
 *     *loss = c * sum_{u,t} <X_u, X_neg(u,t)> - <X_u, X_tg(t)>          (c = 1 / (n_real * T) gives the reference's mean)
 *     G     = d loss / d X on every row of X (rows of fake users n_real <= r < n_user_rows: zero)
 *     w_sfa (optional, [n_user_rows + n_items]) = how often each row occurs in H = cat(users, positives, negatives) of CLeaR.py:98-103: T per real
 *             user, n_real per target occurrence, the negatives' histogram -- the row weights of arl_sfa_l1_fwd_bwd_f32.
 * Deterministic: the item-side sums run in 64-bit fixed point (integer addition is associative; scale chosen on the device so that no sum can
 * overflow, resolution far below fp32 rounding of the same sum); no float atomics, no sort.  top_idx entries must be item ids in [0, n_items)
 * (the caller's own arl_score_mask_topk_f32 output).  1 <= T <= 64, k >= T, d <= 256 with d % 4 == 0, X and G 16-byte aligned,
 * n_items <= 8192 * 128 (d <= 128) or 8192 * 64 (d = 256). */
int64_t arl_cw_topk_term_workspace_bytes(int64_t n_items, int64_t d, int64_t n_real, int64_t n_targets);
int arl_cw_topk_term_f32(const float *X, int64_t n_user_rows, int64_t n_items, int64_t d, int64_t n_real, const int32_t *top_idx, int64_t k,
                         const int64_t *targets, int64_t n_targets, float c, float *G, float *loss, float *w_sfa, void *workspace,
                         arl_stream_t stream);
/* Per-row top-n -> {0,1} rows (+ indices, descending value, ties ascending column).  Replaces project()
 * (attack/White/PGA.py:153-158, CLeaR.py:161-166, DLAttack.py:127-132).  scratch: [rows*cols] fp32. */
int arl_topn_project_rows_f32(const float *M, int64_t rows, int64_t cols, int64_t n, float *out, int32_t *idx,
                              float *scratch, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * All-rows InfoNCE -- replaces the nA x nV logit matrices of recommender/NCL.py:96-115 (ssl_layer_loss: F.normalize, two
 * torch.matmul against ALL users / items, exp, sum, log) and attack/White/InfoAttack.py:214-230, forward and backward, without ever
 * storing a logit.  A [nA, d] and V [nV, d] are row-NORMALISED fp32 tables (|<a, v>| <= 1 is what makes the fixed shift of the
 * log-sum-exp safe), d in {16, 32, 64, 128}.
 *   arl_nce_allrows_lse_f32   lse[b] = log sum_j exp(<a_b, v_j> / tau)
 *   arl_nce_allrows_grad_f32  dA[b] = sum_j P_bj v_j,  dV[j] = sum_b P_bj a_b  with  P_bj = exp(<a_b, v_j>/tau - lse[b])
 *                             (the caller applies 1/tau, the positive pairs' -v_idx / -a_b terms and the upstream gradient);
 *                             dA or dV may be NULL when only one side is differentiated (InfoAttack: the other view is a constant).
 *                             lse_given != 0: lse is an input (from arl_nce_allrows_lse_f32).  lse_given == 0: lse is an OUTPUT of the
 *                             dA pass (dA required), which then accumulates unnormalised exp((s - 1)/tau) terms and divides in the fold:
 *                             forward + backward in two passes over the table instead of three.
 * Exact fp32 products on the matrix cores (v_mfma_f32_16x16x4_f32); partial results are combined in a fixed order (deterministic).
 * workspace: arl_nce_allrows_workspace_bytes(nA, nV, d) bytes, 16-byte aligned like A, V and dA.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_nce_allrows_workspace_bytes(int64_t nA, int64_t nV, int64_t d);
int arl_nce_allrows_lse_f32(const float *A, int64_t nA, const float *V, int64_t nV, int64_t d, float tau, float *lse,
                            void *workspace, arl_stream_t stream);
int arl_nce_allrows_grad_f32(const float *A, int64_t nA, const float *V, int64_t nV, int64_t d, float tau, float *lse, int32_t lse_given,
                             float *dA, float *dV, void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * SSL4Rec's contrastive term, forward and backward in one call -- replaces recommender/SSL4Rec.py:232-247 (item_encoding: two
 * nn.Dropout(p) views of the batch's propagated user rows and of its positive-item rows; cal_cl_loss: InfoNCE of each pair) and the
 * autograd of util/loss.py:42-49.  Xu, Xp [n, d]: the compact rows of the two sides (duplicate positions kept, never merged).  Per side:
 *   V1 = X * M1 * s, V2 = X * M2 * s, s = 1 / (1 - p);  a = V1 / max(||V1||, 1e-12), b = V2 / max(||V2||, 1e-12)   (row-wise)
 *   loss[side] = mean_i( log sum_j exp(<a_i, b_j> / tau) - <a_i, b_i> / tau )          (loss[0]: users, loss[1]: positives)
 *   G[i] += upstream * s * (M1 * dL/dV1 + M2 * dL/dV2)                                   (Gu for the users, Gp for the positives; per position)
 * Mask bit of (side, view, position i, column k) with sv = 2 * side + view:
 *   masks != NULL: bit b = (sv * n + i) * d + k of the packed words, (masks[b >> 5] >> (b & 31)) & 1   ([2 sides][2 views][n][d] bits);
 *   masks == NULL: kept iff (splitmix64(key ^ (((sv << 32) + i) * d + k)) >> 40) * 2^-24 >= p, where key is the hash of (seed, stream_id)
 *                  that arl_simgcl_perturb_rng_f32 forms:  key = splitmix64(seed ^ (stream_id * 0x9E3779B97F4A7C15)).
 * The n x n logits are never stored: the products run on the all-rows InfoNCE kernels (exact fp32 MFMA, fixed log-sum-exp shift, hence
 * tau >= 0.023), the streamed view split so that B = 2048 fills the chip, partials folded in a fixed order; no float atomics, so two
 * calls give bit-identical outputs.  d in {16, 32, 64, 128} (else ARL_E_DIM); 0 <= p < 1, n <= 2^31 / 128 and 16-byte aligned
 * Xu, Xp, Gu, Gp, workspace (else ARL_E_ARG).  workspace: arl_ssl_dropout_nce_workspace_bytes(n, d) bytes.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_ssl_dropout_nce_workspace_bytes(int64_t n, int64_t d);
int arl_ssl_dropout_nce_f32(const float *Xu, const float *Xp, int64_t n, int64_t d, float p, float tau, float upstream, uint64_t seed,
                            uint64_t stream_id, const uint32_t *masks, float *Gu, float *Gp, float *loss, void *workspace, arl_stream_t stream);

/* F.normalize(x, dim=1) of a whole table and its autograd in one pass each (the normalisations around the all-rows InfoNCE,
 * recommender/NCL.py:98-99, 110-111; d % 4 == 0, d <= 256, 16-byte aligned tables):
 *   Y = X / max(||X_r||, 1e-12), nrm[r] = max(||X_r||, 1e-12);   dX = scale * (dY - Y <Y, dY>) / nrm  (dX may alias dY;
 *   scale_dev, optional: a device scalar multiplied into scale -- the upstream gradient without a host round trip). */
int arl_normalize_rows_f32(const float *X, int64_t n, int64_t d, float *Y, float *nrm, arl_stream_t stream);
int arl_normalize_rows_bwd_f32(const float *Y, const float *nrm, const float *dY, int64_t n, int64_t d, float scale, const float *scale_dev,
                               float *dX, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * AUSH's GAN (attack/Gray/AUSH.py; arlib_amd/csrc/arl_gan.hip).  G: Y = sigmoid(relu(T W1^T + b1) W2^T + b2) over an F x S template T,
 * D(x) = sigmoid(x w_D + b_D).  Every operand with F x S or S x S elements must stay within 2^31 - 1 elements (else ARL_E_RANGE).
 *
 * arl_gan_gemm_f32: C [M, N] (row-major, ld N) = sum_k A(m, k) B(k, n), A(m, k) = A[m * sam + k * sak], B(k, n) = B[k * sbk + n * sbn];
 *   sak or sam must be 1, sbn or sbk must be 1 (else ARL_E_ARG).  epilogue 0: C = acc; 1: C = sigmoid(acc + bias[n]); 2: C = aux[m, n] > 0 ?
 *   acc : 0 (aux [M, N]).  Exact fp32 products on v_mfma_f32_16x16x4_f32, the whole K range per output tile in ascending order: deterministic.
 * arl_gan_spmm_f32: out [n_rows, N] = (bias ? bias[n] : 0) + sum_{k in row r} val[k] X[col[k], :] (X row-major [*, N]), then relu if asked;
 *   entries summed in CSR order (int64 rowptr, int32 col).
 * arl_gan_transpose_f32: At [Cn, R] = A [R, Cn]^T (A != At).
 * arl_gan_rows_f32: per row of Y and the dense template Td ([F, S]): rows [F, 4] = (Y_r.w_D, Td_r.w_D, sum (Y - Td)^2, sum over the last T
 *   columns of (1 - Y)); then, in one fixed-order workgroup, losses [3] = (loss1 = -(mean log D(Td) + mean log(1 - D(Y))),
 *   loss2 = mean log D(Td) + mean log(1 - D(Y)) + mean_r s_r^2 + mean (Y - Td)^2, dloss1/db_D), coef [2 F] = (-(1 - D(Td_r)) / F,
 *   D(Y_r) / F) and pf [F] = D(Y_r).  b_D is a device scalar.
 * arl_gan_dz2_f32: dZ2 = dloss2/dY * Y (1 - Y) with dloss2/dY = 2 (Y - Td) / (F S) - (2 s_r / F) [c >= S - T] - (pf_r / F) w_D[c].
 * arl_gan_colsum_f32: out [S] = sum_r (wa ? wa[r] : 1) A[r, :] + (Bm ? wb[r] Bm[r, :] : 0) over F rows, in chunks of 64 rows folded in
 *   ascending order; workspace: arl_gan_colsum_workspace_bytes(F, S) bytes.
 * arl_gan_template_i32: the template of one step.  Row r takes the entries of interaction row user_set[r] (CSR with ascending columns)
 *   whose item c has pos[c] >= 0, in that row's order: column j = pos[c], value = interact[r, j] * mask(r, j) (row r and position j read as
 *   a user and an item id, as the reference does; explicit zeros kept).  mask(r, j) = mask[r * S + j] when mask != NULL, else
 *   1 iff (splitmix64(key ^ (r * 2^32 + items[j])) >> 40) * 2^-24 < item_p[items[j]] with key = arl_gan_hash_key(seed, call).
 *   Count pass (out_ptr NULL): counts[F].  Fill pass: out_ptr [F + 1] row offsets, writes out_col / out_val.
 * arl_gan_hash_mask_u8: out [F, S] = mask(r, j) of the counter hash above.
 * arl_gan_threshold_f32: count pass (out_ptr NULL): counts[r] = #{c : Y[r, c] > thr}; fill pass: ascending columns per row into out_col.
 * ---------------------------------------------------------------------------------------------- */
int arl_gan_gemm_f32(int64_t M, int64_t N, int64_t K, const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C,
                     int32_t epilogue, const float *bias, const float *aux, arl_stream_t stream);
int arl_gan_spmm_f32(int64_t n_rows, int64_t N, const int64_t *rowptr, const int32_t *col, const float *val, const float *X, const float *bias,
                     int32_t relu, float *out, arl_stream_t stream);
int arl_gan_transpose_f32(const float *A, int64_t R, int64_t Cn, float *At, arl_stream_t stream);
int arl_gan_rows_f32(const float *Y, const float *Td, int64_t F, int64_t S, int64_t T, const float *wD, const float *bD, float *rows, float *losses,
                     float *coef, float *pf, arl_stream_t stream);
int arl_gan_dz2_f32(const float *Y, const float *Td, const float *rows, const float *pf, const float *wD, int64_t F, int64_t S, int64_t T, float *dZ2,
                    arl_stream_t stream);
int64_t arl_gan_colsum_workspace_bytes(int64_t F, int64_t S);
int arl_gan_colsum_f32(const float *A, const float *wa, const float *Bm, const float *wb, int64_t F, int64_t S, float *out, void *workspace,
                       arl_stream_t stream);
uint64_t arl_gan_hash_key(uint64_t seed, uint64_t call);
int arl_gan_template_i32(int64_t F, int64_t S, int64_t n_users, const int32_t *user_set, const int64_t *rowptr, const int32_t *col, const float *val,
                         const int32_t *pos, const int32_t *items, const uint8_t *mask, const float *item_p, uint64_t seed, uint64_t call,
                         const int64_t *out_ptr, int64_t *counts, int32_t *out_col, float *out_val, arl_stream_t stream);
int arl_gan_hash_mask_u8(int64_t F, int64_t S, const int32_t *items, const float *item_p, uint64_t seed, uint64_t call, uint8_t *out,
                         arl_stream_t stream);
int arl_gan_threshold_f32(const float *Y, int64_t F, int64_t S, float thr, const int64_t *out_ptr, int64_t *counts, int32_t *out_col,
                          arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * LegUP's ranking loss (csrc/arl_colsoftmax.hip; reference attack/Gray/LegUP.py:160-171) -- a softmax over the USERS of every item column
 * of s = Pu Pi^T [U, I], which is never stored.  Pu [U, d], Pi [I, d], d in {16, 32, 64, 128}, 16-byte aligned; targets: T device column
 * ids in [0, I) (1 <= T <= 1024; a repeated id counts as often as it is listed).
 *   lse [I]  : lse[i] = log sum_u exp(s[u, i]), with a running maximum
 *   loss [1] : -(I * sum_u sum_t s[u, c_t] - U * T * sum_i lse[i])  =  -sum_{u, t, i} (s[u, c_t] - lse[i])
 *   dPu [U, d], dPi [I, d] (each optional, NULL = skipped): the loss's gradients.
 * Fixed-order reductions: bit-identical from run to run.  The workspace needs no initialisation. */
int64_t arl_colsoftmax_target_workspace_bytes(int64_t U, int64_t I, int64_t d, int32_t want_dPi);
int arl_colsoftmax_target_loss_f32(const float *Pu, int64_t U, const float *Pi, int64_t I, int64_t d, const int32_t *targets, int64_t T, float *lse,
                                   float *loss, float *dPu, float *dPi, void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GSPAttack's L_per (csrc/arl_allpairs.hip; reference attack/Black/GSPAttack.py:63-75) -- a binary cross-entropy over every score of
 * s = Pu Pi^T [R, I], which is never stored, against a sparse target matrix.  Pu [R, d], Pi [I, d], d in {16, 32, 64, 128}, 16-byte aligned,
 * rows of either table <= (2^31 - 1) / 128.  With f0(s) = -log(sigmoid(-s) + eps), f1(s) = -log(sigmoid(s) + eps):
 *   pos_rowptr [R + 1], pos_col [nnz], pos_val [nnz] | NULL (all 1): the positives (r, c) with weights a, CSR by row, int32; a repeated
 *     entry counts as often as it is listed.  post_rowptr [I + 1], post_col [nnz] (row ids), post_perm [nnz] | NULL: the same set by item,
 *     post_perm mapping its entries to pos_val (needed with pos_val); read only when dPi is wanted.
 *   rowloss [R] : sum_i f0(s[r, i]) + sum_{(r, c) listed} a (f1 - f0)(s[r, c])          (unweighted)
 *   loss [1]    : sum_r row_weight[r] rowloss[r]                                        (accumulated in double)
 *   dPu [R, d], dPi [I, d] (each optional, NULL = skipped): gradients of upstream * loss.
 * Fixed-order reductions, no atomics: bit-identical from run to run, and the loss-only call gives the bits of the gradient call.  The
 * workspace (arl_bce_allpairs_workspace_bytes; 0 for a shape outside the limits) needs no initialisation. */
/* attack/Black/GSPAttack.py:63-75 */
int64_t arl_bce_allpairs_workspace_bytes(int64_t R, int64_t I, int64_t d, int32_t want_grad);
/* attack/Black/GSPAttack.py:63-75 */
int arl_bce_allpairs_f32(const float *Pu, int64_t R, const float *Pi, int64_t I, int64_t d, const int32_t *pos_rowptr, const int32_t *pos_col,
                         const float *pos_val, const int32_t *post_rowptr, const int32_t *post_col, const int32_t *post_perm,
                         const float *row_weight, float eps, float upstream, float *rowloss, float *loss, float *dPu, float *dPi, void *workspace,
                         arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Full-ranking attack metrics: the rank of each target item for each user (csrc/arl_targetrank.hip; the sufficient statistic of the
 * reference's AttackMetric, util/metrics.py:125-208).  Pu [U, d], Pi [I, d] fp32, 16-byte aligned; targets [T] int32, distinct, in [0, I).
 * With s = Pu Pi^T in exact fp32 (one instruction sequence for every score that is compared):
 *   rank [U, T] int32 : #{ j != targets[t], (u, j) not masked : s[u, j] > s[u, targets[t]] or (equal and j < targets[t]) }, the 0-based
 *                       position of the target in user u's descending row with ties broken by item id; -1 where (u, targets[t]) is masked
 *   tscore [U, T] fp32: s[u, targets[t]], the thresholds the counts were taken against
 *   mask_rowptr [U + 1], mask_col [nnz] | both NULL: pairs left out of the count, CSR by user, int32, each row sorted and distinct.
 * Limits: d in {16, 32, 64, 128}, 1 <= T <= 64, 1 <= U, I <= (2^31 - 1) / 128; anything else is ARL_E_RANGE.  Integer counts, no atomics:
 * bit-identical from run to run.  The workspace (arl_target_rank_workspace_bytes; 0 when the item stream is not split or the shape is
 * outside the limits) needs no initialisation. */
/* util/metrics.py:125-208 */
int64_t arl_target_rank_workspace_bytes(int64_t U, int64_t I, int64_t d, int64_t T);
/* util/metrics.py:125-208 */
int arl_target_rank_f32(const float *Pu, int64_t U, const float *Pi, int64_t I, int64_t d, const int32_t *targets, int64_t T,
                        const int32_t *mask_rowptr, const int32_t *mask_col, int32_t *rank, float *tscore, void *workspace,
                        arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GSPAttack's profile generator (csrc/arl_profilegen.hip; reference attack/Black/GSPAttack.py:120-130, 201-202, 224-231 as repaired in
 * arlib_amd/attack/Black/GSPAttack.py).  Every pointer 16-byte aligned; ARL_E_DIM for H > 1024 or k > 512, ARL_E_RANGE for F or I outside
 * the kernels' grids (F <= 524 280 for the pair MLP, I <= 2^31 - 2049, F * ceil(I / 256) [* k for the noise] < 2^31), ARL_E_ARG for an
 * empty or misaligned argument, k > I or tau <= 0; all checked before any launch.  No atomics, fixed-order reductions: bit-identical from
 * run to run.  No workspace needs initialisation.
 *
 * Pair-MLP head: A [F, H], B [I, H], w2 [H], b2 [1] (device) -> x [F, I], x[f, i] = b2 + sum_h w2[h] relu(A[f, h] + B[i, h]); the
 * Linear(2d, H) - ReLU - Linear(H, 1) of the reference on cat(e_f, e_i) with A = E_f W1[:, :d]^T + b1 and B = E_i W1[:, d:]^T.  No
 * F x I x H tensor exists.  Backward for an upstream g [F, I] (the ReLU derivative at exactly 0 is 0):
 *   dA[f, h] = w2[h] sum_i g[f, i] [A[f, h] + B[i, h] > 0],   dB[i, h] = w2[h] sum_f g[f, i] [A[f, h] + B[i, h] > 0],
 *   dw2[h] = sum_{f, i} g[f, i] relu(A[f, h] + B[i, h]),      db2 [1] = sum g;       sums in fp32 per tile, in double across tiles. */
/* attack/Black/GSPAttack.py:120-130 */
int arl_pair_mlp_fwd_f32(const float *A, int64_t F, const float *B, int64_t I, int64_t H, const float *w2, const float *b2, float *x, arl_stream_t stream);
/* attack/Black/GSPAttack.py:120-130 */
int64_t arl_pair_mlp_workspace_bytes(int64_t F, int64_t I, int64_t H);
/* attack/Black/GSPAttack.py:120-130 */
int arl_pair_mlp_bwd_f32(const float *g, const float *A, int64_t F, const float *B, int64_t I, int64_t H, const float *w2, float *dA, float *dB, float *dw2,
                         float *db2, void *workspace, arl_stream_t stream);
/* Relaxed Gumbel top-k: x [F, I] finite, 1 <= k <= I, tau > 0.  Round r, over the items not picked in earlier rounds: z = (x + g_r) / tau,
 * y_r = softmax(z) over the items, j_r = argmax z (the lowest index on an exact tie).
 *   S [F, I] = sum_r y_r,  picks [F, k] int32,  lse [F, k] the per-round log-sum-exp,  stats [F, k, 2] the per-round (max z, sum exp(z - max)).
 * noise [k, F, I] is the caller's g; NULL: g = -log(-log u), u in (0, 1) from 24 bits of a splitmix64 counter hash of
 * (seed, call, r, f, i) -- a function of those five numbers only.  arl_gumbel_noise_f32 writes that draw out as [k, F, I].
 * Backward (the argmax detached): dx[f, i] = (1 / tau) sum_r y_r[i] (dS[f, i] - sum_j y_r[j] dS[f, j]), y_r recomputed from x, the noise,
 * picks and stats.  Workspace: forward F * ceil(I / 32) words, backward F * ceil(I / 256) * k + F * k floats. */
/* attack/Black/GSPAttack.py:201-202, 224-231 */
int64_t arl_gumbel_topk_workspace_bytes(int64_t F, int64_t I, int64_t k, int32_t backward);
/* attack/Black/GSPAttack.py:201-202, 224-231 */
int arl_gumbel_topk_fwd_f32(const float *x, int64_t F, int64_t I, int64_t k, float tau, const float *noise, uint64_t seed, uint64_t call, float *S, int32_t *picks,
                            float *lse, float *stats, void *workspace, arl_stream_t stream);
/* attack/Black/GSPAttack.py:201-202, 224-231 */
int arl_gumbel_topk_bwd_f32(const float *x, int64_t F, int64_t I, int64_t k, float tau, const float *noise, uint64_t seed, uint64_t call, const int32_t *picks,
                            const float *stats, const float *dS, float *dx, void *workspace, arl_stream_t stream);
/* attack/Black/GSPAttack.py:201-202, 224-231 */
int arl_gumbel_noise_f32(uint64_t seed, uint64_t call, int64_t k, int64_t F, int64_t I, float *out, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * PoisonRec's policy head (csrc/arl_policyhead.hip; reference attack/Black/PoisonRec.py:363-371, 398-401) -- a Bernoulli distribution over
 * every item whose logits are p = softmax_i(q E^T), with no B x I tensor.  q [B, d], E [I, d] fp32, d in {16, 32, 64, 128} (else ARL_E_DIM),
 * 16-byte aligned, B, I >= 1 (else ARL_E_ARG) and <= (2^31 - 1) / 128 (else ARL_E_RANGE).  actions [B, W] int32, W = ceil(I / 32): bit i % 32
 * of word i / 32 is item i; pad bits are written as 0 and never read as items.  With sp = softplus(p), sg = sigmoid(p):
 *   logp [B] = sum_i (a p - sp),   ent [B] = sum_i (sp - p sg)
 *   dq [B, d], dE [I, d] (each optional, NULL = skipped; gl [B], ge [B] are then required): the gradients of sum_b gl[b] logp[b] + ge[b] ent[b],
 *     dz_i = p_i (c_i - sum_j p_j c_j) with c_i = gl (a_i - sg_i) - ge p_i sg_i (1 - sg_i), dq = dz E, dE = dz^T q.
 * eval: four streamed passes (row max and sum, row sums, dq, dE).  sample: the first pass, then a_i = (u_i < sg_i) with u the caller's
 * [B, I] tensor or, u NULL, u = n 2^-24 from 24 bits of the splitmix64 counter hash of (seed, call, row0 + b, i); deterministic != 0:
 * a_i = (p_i > 0), which is sg_i > 1/2.  It writes the packed actions, logp and count [B] (the set bits per row).
 * arl_bernoulli_uniforms_f32 writes the hash's draw out as [B, I].  No atomics, fixed-order reductions: bit-identical from run to run.
 * The workspace (arl_bernoulli_softmax_workspace_bytes, want_grad = 1 when dq or dE is asked for; 0 for a shape outside the limits) needs
 * no initialisation. */
/* attack/Black/PoisonRec.py:363-371, 398-401 */
int64_t arl_bernoulli_softmax_workspace_bytes(int64_t B, int64_t I, int64_t d, int32_t want_grad);
/* attack/Black/PoisonRec.py:363-371, 398-401 */
int arl_bernoulli_softmax_eval_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const int32_t *actions, const float *gl, const float *ge,
                                   float *logp, float *ent, float *dq, float *dE, void *workspace, arl_stream_t stream);
/* attack/Black/PoisonRec.py:363-371, 398-401 */
int arl_bernoulli_softmax_sample_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const float *u, uint64_t seed, uint64_t call, int64_t row0,
                                     int32_t deterministic, int32_t *actions, float *logp, int32_t *count, void *workspace, arl_stream_t stream);
/* attack/Black/PoisonRec.py:363-371, 398-401 */
int arl_bernoulli_uniforms_f32(uint64_t seed, uint64_t call, int64_t row0, int64_t B, int64_t I, float *out, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The multinomial likelihood of the autoencoder recommenders (csrc/arl_multinomial.hip; Mult-DAE / Mult-VAE, Liang et al., WWW'18; no counterpart
 * in the reference) -- a softmax over every item for each batch row, read at the row's positives, with no B x I tensor.  q [B, d] the rows'
 * last activations, E [I, d] the output-layer weight, fp32; the positives as CSR (rowptr [B + 1], col [nnz] int32, sorted and distinct within a
 * row, val [nnz] fp32 weights w | NULL: every w is 1), g [B] the per-row upstream.  With z = q E^T, lse_b = log sum_i exp z_bi,
 * n_b = sum_{i in pos(b)} w_bi and p = softmax_i(z):
 *   nll[b] = n_b lse_b - sum_{i in pos(b)} w_bi z_bi
 *   dq[b]  = g_b ( n_b sum_i p_bi E_i - sum_{i in pos(b)} w_bi E_i )
 *   dE[i]  = sum_b g_b ( n_b p_bi - w_bi [i in pos(b)] ) q_b
 * A row without positives gives nll = 0 and contributes nothing to either gradient.  nll [B] and lse [B] are always written; dq [B, d] and
 * dE [I, d] are each written when not NULL and then need g.  dE also needs the positives by item: trowptr [I + 1], tcol [nnz] the row ids, and with
 * val tperm [nnz], the entries' positions in the by-row arrays.  The index arrays are trusted.
 * d in {16, 32, 64, 128} (else ARL_E_DIM), B, I >= 1 and nnz >= 0 (else ARL_E_ARG), B, I <= (2^31 - 1) / 128 and nnz < 2^31 (else ARL_E_RANGE),
 * q, E, dq, dE and the workspace 16-byte aligned (else ARL_E_ARG); a missing pointer is ARL_E_NULL; all checked before any launch.  Exact fp32
 * products on v_mfma_f32_16x16x4_f32, an online maximum for the log-sum-exp, no atomics and fixed-order sums: bit-identical from run to run.
 * The workspace (arl_multinomial_softmax_workspace_bytes, want_grad = 1 when dq or dE is asked for; 0 for a shape outside the limits) needs
 * no initialisation. */
int64_t arl_multinomial_softmax_workspace_bytes(int64_t B, int64_t I, int64_t d, int32_t want_grad);
int arl_multinomial_softmax_f32(const float *q, int64_t B, const float *E, int64_t I, int64_t d, const int32_t *rowptr, const int32_t *col, const float *val, int64_t nnz,
                                const int32_t *trowptr, const int32_t *tcol, const int32_t *tperm, const float *g, float *nll, float *lse, float *dq, float *dE,
                                void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Alternating least squares for implicit feedback (csrc/arl_als.hip; WRMF as published, Hu, Koren, Volinsky, ICDM'08; the reference's WRMF is
 * a sampled SGD approximation and is untouched).  Y [n, d] the OTHER table, fp32; the rows to solve as CSR (rowptr [n_rows + 1], col [nnz] int32
 * in [0, n), val [nnz] fp32 weights w | NULL: every w is 1).  With p = 1 on the stored entries and confidence c = 1 + alpha w:
 *   L   = sum_u sum_i c_ui (p_ui - x_u . y_i)^2 + lambda (|X|^2 + |Y|^2)          over ALL (u, i)
 *   G   = Y^T Y                                                                   (arl_als_gram_f64: d x d, double)
 *   A_r = G + alpha sum_{i in P_r} w_ri y_i y_i^T + lambda I,   b_r = sum_{i in P_r} (1 + alpha w_ri) y_i,   x_r = A_r^-1 b_r     (arl_als_solve_rows_f32)
 *   L   = sum_u [ x_u^T G x_u + sum_{i in P_u} ((1 + alpha w)(1 - s)^2 - s^2) ] + lambda (|X|^2 + |Y|^2),   s = x_u . y_i         (arl_als_objective_f64)
 * gram      : G [d, d] double, summed over at most 256 fixed spans of rows in ascending order (products of fp32 values are exact in double).
 * solve_rows: X [n_solve, d]: row j is the solution of CSR row rows[j] (rows [n_solve] int32 in [0, n_rows), repeats allowed) or of row j when
 *             rows is NULL (then n_solve = n_rows).  nnz_listed = the listed rows' entries in total (nnz without rows; it sizes the workspace).
 *             The rank-n_r update runs exact fp32 on v_mfma_f32_16x16x4_f32 over the lower-triangular tiles (a stage of 64 entries in fp32, the
 *             stages in double), A_r is completed, factorised and solved in double.  A row longer than split_len (<= 0: the default,
 *             arl_als_default_split_len) is cut into pieces of split_len entries, accumulated by separate workgroups and added in piece order;
 *             a row without entries gives exactly 0.  alpha, lambda >= 0 (lambda > 0 keeps A_r positive definite whatever the row).
 * objective : out [1] double; X [n_rows, d] the rows' table, G the Gram matrix of Y; no n_rows x n score matrix.
 * d in {16, 32, 64, 128} (else ARL_E_DIM), sizes >= 1 (else ARL_E_ARG), n, n_rows, n_solve <= (2^31 - 1) / 128 and nnz_listed < 2^31 (else
 * ARL_E_RANGE), tables, G and workspaces 16-byte aligned (else ARL_E_ARG); a missing pointer is ARL_E_NULL; all checked before any launch.  The
 * index arrays are trusted.  No atomics, fixed-order sums: bit-identical from run to run (for a given split_len).  The workspaces
 * (*_workspace_bytes; 0 for a shape outside the limits) need no initialisation. */
int64_t arl_als_default_split_len(void);
int64_t arl_als_gram_workspace_bytes(int64_t n, int64_t d);
int arl_als_gram_f64(const float *Y, int64_t n, int64_t d, double *G, void *workspace, arl_stream_t stream);
int64_t arl_als_solve_rows_workspace_bytes(int64_t n_solve, int64_t nnz_listed, int64_t d, int64_t split_len);
int arl_als_solve_rows_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                           const int32_t *rows, int64_t n_solve, int64_t nnz_listed, double alpha, double lambda, int64_t split_len, float *X, void *workspace,
                           arl_stream_t stream);
int64_t arl_als_objective_workspace_bytes(int64_t n_rows, int64_t n, int64_t d);
int arl_als_objective_f64(const float *X, int64_t n_rows, const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col,
                          const float *val, double alpha, double lambda, double *out, void *workspace, arl_stream_t stream);

/* The row solve under a target rule, and its adjoint (csrc/arl_als.hip; the operator an attack needs to differentiate through ALS sweeps, as in Tang,
 * Wen, Wang, RecSys'20).  b_r = sum_{i in P_r} beta(w_ri) y_i with
 *   ARL_ALS_TARGET_STORED : beta(w) = 1 + alpha w      (arl_als_solve_rows_f32: the same launches, the same bits)
 *   ARL_ALS_TARGET_RELAXED: beta(w) = (1 + alpha) w    (the same double at w = 1; an entry of weight 0 contributes nothing, as if it were absent)
 * solve_rows_target: arl_als_solve_rows_f32 with the rule selectable; arguments, limits and workspace as there.
 * adjoint: given X [n_rows, d] = the solved rows (all of them, in row order) and gX [n_rows, d] = dL/dX, with z_r = A_r^-1 g_r, s = x_r . y_i,
 *   t = z_r . y_i and C = sum_r z_r x_r^T:
 *     dval[e] = t (beta'(w) - alpha s)                                                        beta' = alpha | 1 + alpha       (dval NULL: skipped)
 *     dY[i]   = sum_{r with i} [ (beta(w_ri) - alpha w_ri s) z_r - alpha w_ri t x_r ] - y_i (C + C^T)      (the last term: the path through G = Y^T Y)
 *   A_r is rebuilt and factorised as in the forward (exact fp32 MFMA tiles, double from there on) with g_r travelling where b_r travels; s and t are
 *   double dots; C is summed in double over the fixed spans of the Gram kernel; dY[i] runs over the entries of column i in the transposed order
 *   (tptr [n + 1], trow [nnz] the row ids, tperm [nnz] the entries' positions in the by-row arrays), in double, a column longer than col_split_len
 *   (<= 0: arl_als_default_col_split_len) cut into pieces added in piece order.  A row without entries has z = 0 and contributes nothing whatever gX
 *   holds.  nnz >= 1.  No atomics, one writer per word, fixed orders: bit-identical from run to run (for given split lengths); no n_rows x d x d
 *   stack.  workspace: arl_als_adjoint_workspace_bytes (0 outside the limits), no initialisation needed.  Limits and error codes as above. */
#define ARL_ALS_TARGET_STORED 0
#define ARL_ALS_TARGET_RELAXED 1
int64_t arl_als_solve_rows_target_workspace_bytes(int64_t n_solve, int64_t nnz_listed, int64_t d, int64_t split_len);
int arl_als_solve_rows_target_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val,
                                  int64_t n_rows, const int32_t *rows, int64_t n_solve, int64_t nnz_listed, double alpha, double lambda, int32_t target,
                                  int64_t split_len, float *X, void *workspace, arl_stream_t stream);
int64_t arl_als_default_col_split_len(void);
int64_t arl_als_adjoint_workspace_bytes(int64_t n, int64_t n_rows, int64_t nnz, int64_t d, int64_t split_len, int64_t col_split_len);
int arl_als_adjoint_f32(const float *Y, int64_t n, int64_t d, const double *G, const int32_t *rowptr, const int32_t *col, const float *val, int64_t n_rows,
                        int64_t nnz, const float *X, const float *gX, const int32_t *tptr, const int32_t *trow, const int32_t *tperm, double alpha,
                        double lambda, int32_t target, int64_t split_len, int64_t col_split_len, float *dY, float *dval, void *workspace,
                        arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Lloyd's k-means for NCL's prototypes (csrc/arl_kmeans.hip).  Replaces recommender/NCL.py:52-73 (e_step / run_kmeans: sklearn's KMeans on
 * host copies of the tables; the commented faiss.Kmeans(gpu=True) of :61-66 is what the authors meant).  X [N, d] points, C [k, d]
 * centroids, d in {16, 32, 64, 128} (else ARL_E_DIM), N, k >= 1 (else ARL_E_ARG) and <= 2^31 / 128 (else ARL_E_RANGE), X, C and
 * workspaces 16-byte aligned (else ARL_E_ARG).  No N x k matrix is stored, no float atomics: every output is bit-identical from run to run.
 *   assign : labels[n] = argmax_c (<x_n, c> - 1/2 |c|^2) = the nearest centroid, score[n] = that maximum; exact fp32 products on
 *            v_mfma_f32_16x16x4_f32.  Equal scores: the LOWER index.  A point whose scores are all NaN: label 0 (never out of range).
 *            bias [k]: scratch, receives -1/2 |c|^2.
 *   update : C_new[c] = mean of the rows labelled c, or C_prev[c] bit for bit for a cluster without members.  The membership comes from the
 *            caller: order [N] = row ids stably sorted by label, seg_ptr [k + 1] = first position of every cluster in `order`,
 *            chunk_ptr [k + 1] = exclusive prefix sum of ceil(count_c / arl_kmeans_chunk_rows).  A cluster's rows are summed in ascending
 *            order in chunks of that many rows, the chunks folded in order, the sum divided by the count.  C_new must not alias C_prev.
 *   sum    : out[0] = sum of v[0..n) (squared != 0: of v^2) in double over fixed spans -- the two terms of the inertia
 *            sum |x|^2 - 2 sum score.  workspace: arl_kmeans_sum_workspace_bytes bytes, 8-byte aligned like out.
 * ---------------------------------------------------------------------------------------------- */
int arl_kmeans_assign_f32(const float *X, int64_t N, const float *C, int64_t k, int64_t d, float *bias, int32_t *labels, float *score,
                          arl_stream_t stream);
int64_t arl_kmeans_chunk_rows(void);
int64_t arl_kmeans_update_workspace_bytes(int64_t N, int64_t k, int64_t d);
int arl_kmeans_update_f32(const float *X, int64_t N, int64_t d, const int32_t *order, const int32_t *seg_ptr, const int32_t *chunk_ptr, int64_t k,
                          const float *C_prev, float *C_new, void *workspace, arl_stream_t stream);
int64_t arl_kmeans_sum_workspace_bytes(void);
int arl_kmeans_sum_f64(const float *v, int64_t n, int32_t squared, double *out, void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Greedy k-means++ start for the k-means above (csrc/arl_kmeans.hip): sklearn's _kmeans_plusplus with unit weights, no host read inside the loop.
 * State: closest [N] = squared distance of every row to its nearest chosen centre, pot = sum closest.  Step c = 1 .. k - 1: candidate t < n_trials
 * is the first row whose inclusive running sum of closest reaches u[c - 1][t] * pot (row N - 1 if none does), mins[t][n] = min(closest[n],
 * |x_n - x_cand_t|^2) as a direct sum of squared differences, pot_t = sum mins[t] in double over fixed spans; the lowest t with the smallest pot_t wins.
 * Limits as above; n_trials in 1 .. 16 (else ARL_E_ARG), k <= N (else ARL_E_ARG).  Ids read from device memory are clamped into [0, N).
 *   spans  : the number of row spans S of a table of N rows (the second extent of `part`) and the rows of a span (span b = rows [b rows, (b + 1) rows));
 *            0 for N outside the limits.
 *   dist   : one distance pass.  cand_ids [n_cand] (device), closest [N] or NULL (= +inf: the pass that forms closest from the first centre),
 *            mins [n_cand][N], part [n_cand][S] double.
 *   pick   : winner[0] = the winning t, winner[1] = its row, cand_pot [n_cand] = the folded potentials, closest_out [N] (may be NULL) = the winner's
 *            minima, next_ids [n_next] = the candidates drawn with u [n_next] (n_next = 0: none; 0 .. 16).
 *   whole  : arl_kmeanspp_f32 enqueues all k - 1 steps.  first = the first centre's row, u [(k - 1)][n_trials] double (device; unused for k = 1),
 *            indices [k] int32, closest [N] = the final state, trace (both may be NULL): cand_ids [(k - 1)][n_trials], cand_pot likewise.
 *            workspace: arl_kmeanspp_workspace_bytes(N, n_trials) bytes, 16-byte aligned like X; part, u and cand_pot 8-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_kmeanspp_spans(int64_t N);
int64_t arl_kmeanspp_span_rows(int64_t N);
int64_t arl_kmeanspp_workspace_bytes(int64_t N, int64_t n_trials);
int arl_kmeanspp_dist_f32(const float *X, int64_t N, int64_t d, const int32_t *cand_ids, int64_t n_cand, const float *closest, float *mins, double *part,
                          arl_stream_t stream);
int arl_kmeanspp_pick_f64(const float *mins, const double *part, int64_t N, int64_t n_cand, const int32_t *cand_ids, const double *u, int64_t n_next,
                          int32_t *next_ids, int32_t *winner, double *cand_pot, float *closest_out, arl_stream_t stream);
int arl_kmeanspp_f32(const float *X, int64_t N, int64_t d, int64_t k, int64_t n_trials, int64_t first, const double *u, int32_t *indices, float *closest,
                     int32_t *cand_ids, double *cand_pot, void *workspace, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * DirectAU's two terms (csrc/arl_pairloss.hip), forward and backward in one call each.  Replace util/loss.py:17-23 (alignment_loss,
 * uniformity_loss) and their autograd.  Inputs are RAW rows; the calls normalise them (y = x / max(||x||, 1e-12), as F.normalize).
 *   uniformity : loss[0] = log( mean_{i<j} exp(-t |y_i - y_j|^2) ) over the rows of X [n, d], dX [n, d] (NULL = forward only) = upstream * dloss/dX.
 *                The reference stores n (n - 1) / 2 distances (torch.pdist); here no n x n array exists: dist^2 = max(q_i + q_j - 2 <y_i, y_j>, 0)
 *                with q_r = |y_r|^2 kept per row (a zero row stays zero, rows are not assumed to have unit length), the scores exact fp32 on
 *                v_mfma_f32_16x16x4_f32, the diagonal masked.  The gradient's two sums, rowsum_i = sum_j e_ij and G_i = sum_j e_ij y_j, cancel
 *                in y_i rowsum_i - G_i, so they are summed in DOUBLE: G on v_mfma_f64_16x16x4_f64, at half the fp32 matrix rate (with dX the
 *                call costs about 2.3 times the forward alone, not 2).  The streamed side is cut into arl_uniformity_splits(n) splits whose
 *                partials are summed in split order, the total in double over fixed spans: bit-identical from run to run, no float atomics.
 *                d in {16, 32, 64, 128} (else ARL_E_DIM), n >= 2 and t > 0 (else ARL_E_ARG), n <= 2^31 / 128 (else ARL_E_RANGE), X, dX and the
 *                workspace 16-byte aligned (else ARL_E_ARG).  workspace: arl_uniformity_workspace_bytes(n, d) bytes (0 outside the limits); it
 *                needs no initialisation.
 *   alignment  : loss[0] = mean_b |x^_b - y^_b|^alpha over the row pairs of X, Y [n, d]; dX, dY [n, d] (both or neither) = upstream * dloss/d(X, Y).
 *                A pair with x^_b == y^_b contributes gradient 0 (torch's subgradient of the norm at the origin).  One wave per pair, the mean
 *                summed in double in a fixed order.  d % 4 == 0, d <= 256 (else ARL_E_DIM), n >= 1 and alpha > 0 (else ARL_E_ARG),
 *                n <= 2^31 / 128 (else ARL_E_RANGE), 16-byte aligned tables.  terms [n]: scratch, receives the per-pair terms.
 * ---------------------------------------------------------------------------------------------- */
int64_t arl_uniformity_splits(int64_t n);
int64_t arl_uniformity_workspace_bytes(int64_t n, int64_t d);
int arl_uniformity_fwd_bwd_f32(const float *X, int64_t n, int64_t d, float t, float upstream, float *loss, float *dX, void *workspace,
                               arl_stream_t stream);
int arl_alignment_fwd_bwd_f32(const float *X, const float *Y, int64_t n, int64_t d, float alpha, float upstream, float *loss, float *dX, float *dY,
                              float *terms, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * GOAT's co-rating degree (csrc/arl_corating.hip).  Replaces attack/Gray/GOAT.py:37-39 (interact.T @ interact, every stored entry set to 1,
 * column sums): out[j] = the number of distinct items i (j included) that share a user with item j, 0 for an item nobody rated.  The product
 * is never formed: a workgroup owns one item and a bitmap of n_items bits in LDS, ORs the items of every user of j into it and popcounts.
 *   u_rowptr [n_users + 1], u_col [nnz]     : the interaction matrix as CSR (users -> items; any order within a row, repeats allowed);
 *   i_colptr [n_items + 1], i_row [nnz]     : the same matrix as CSC (items -> users);
 *   order [n_items] (optional, NULL = index order): a permutation of the items, the order in which workgroups take them (heaviest first);
 *   out [n_items] int32: every word is written exactly once; no other global memory is written, no workspace is needed.
 * n_items > arl_corating_max_items() (the 160 KiB of LDS minus the kernel's 16 words, in bits) or n_users >= 2^31: ARL_E_RANGE before any
 * launch.  Ids outside [0, n_users) / [0, n_items) are skipped.  Integer result: bit-identical from run to run. */
int64_t arl_corating_max_items(void);
int arl_corating_degree_i32(const int64_t *u_rowptr, const int32_t *u_col, const int64_t *i_colptr, const int32_t *i_row, int64_t n_users,
                            int64_t n_items, const int32_t *order, int32_t *out, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exact top-k co-occurrence neighbours of the rows of a sparse binary matrix (csrc/arl_cooccur.hip; no reference counterpart: the primitive
 * under the profile detectors of arlib_amd/detect and, on the transposed input, under an item-kNN neighbour list).  X is n_rows x n_cols:
 *   rowptr [n_rows + 1], col [nnz]    : X as CSR; every row a set, columns ascending and distinct within a row (the entry trusts this);
 *   colptr [n_cols + 1], irow [nnz]   : the same matrix column-major, rows ascending within a column;
 *   rows [n_queries] (optional)       : the query rows, any order, repeats allowed; NULL = query q is row q, and n_queries is then n_rows;
 *   order [n_queries] (optional)      : a permutation of the query slots, the order in which workgroups take them (heaviest first);
 *   idx, cnt [n_queries, k] int32     : for query q up to k rows v != u with c = |X_u & X_v| > 0, best first by `measure`, ties to the smaller
 *                                       row id; cnt holds c; unused slots are idx = -1, cnt = 0.  Every word is written exactly once, also
 *                                       for an empty query row or a query id outside [0, n_rows); nothing else is written, no workspace.
 * The order is decided in 64-bit integers (cosine: c1^2 d2 against c2^2 d1; Jaccard: c1 (du + d2 - c2) against c2 (du + d1 - c1)), so the
 * result is a function of the input alone.  max_degree is the largest row degree, stated by the caller: past arl_cooccur_max_degree(measure)
 * (2^20 for cosine, 2^31 - 1 otherwise) the keys could overflow and the entry returns ARL_E_RANGE; the entry trusts the value (it cannot read
 * device memory without a synchronise), and with a max_degree below the true one the order of the lists is unspecified.  1 <= k <= arl_cooccur_max_k() = 128;
 * tile_rows = 0 takes arl_cooccur_default_tile_rows() (16 384 candidate rows = 64 KiB of LDS counters, two workgroups per CU), at most
 * arl_cooccur_max_tile_rows() (36 864).  Negative sizes, k < 1 or an unknown measure: ARL_E_ARG; k, tile_rows, n_rows, n_cols, n_queries,
 * n_queries * k >= 2^31 or max_degree past their limits: ARL_E_RANGE; a NULL rowptr, colptr, idx or cnt with n_queries > 0: ARL_E_NULL; all
 * before any launch.  Ids outside [0, n_rows) / [0, n_cols) are skipped. */
#define ARL_COOCCUR_COUNT 0
#define ARL_COOCCUR_COSINE 1
#define ARL_COOCCUR_JACCARD 2
int64_t arl_cooccur_max_k(void);
int64_t arl_cooccur_max_tile_rows(void);
int64_t arl_cooccur_default_tile_rows(void);
int64_t arl_cooccur_max_degree(int32_t measure);
int arl_cooccur_topk_i32(const int64_t *rowptr, const int32_t *col, const int64_t *colptr, const int32_t *irow, int64_t n_rows, int64_t n_cols,
                         const int32_t *rows, int64_t n_queries, int64_t k, int32_t measure, int64_t max_degree, const int32_t *order,
                         int64_t tile_rows, int32_t *idx, int32_t *cnt, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exact fixed-point item-kNN scores and the full-catalogue top-N (csrc/arl_itemknn.hip; no reference counterpart: the scoring step of
 * arlib_amd/recommender/ItemKNN.py on the neighbour lists arl_cooccur_topk_i32 writes for the transposed matrix).  X is n_users x n_items:
 *   rowptr [n_users + 1], col [nnz]   : X as CSR; every row a set, columns ascending and distinct within a row (the entry trusts this);
 *   nbr_idx, nbr_w [n_items, k] int32 : neighbour r of item j and its non-negative weight; a slot with nbr_idx < 0 is unused, its weight ignored;
 *   rows [n_queries] (optional)       : the query users, any order, repeats allowed; NULL = query q is user q;
 *   tgt_id, tgt_col [n_targets]       : the distinct target items in ascending order and the column of `rank` each one is reported in;
 *   order [n_queries] (optional)      : a permutation of the query slots, the order in which workgroups take them (heaviest first);
 *   idx int32, score int64 [n_queries, n] : s(u, i) = sum over j in X_u, r < k of [nbr_idx[j, r] == i] nbr_w[j, r], exact in 64 bits; every
 *                                       item is a candidate (score 0 included; with mask_profile != 0 the items of X_u are not), ordered by
 *                                       (score descending, id ascending); the n best, best first; unused slots are idx = -1, score = 0;
 *   rank int32 [n_queries, n_targets] : the number of candidates that beat the target, -1 for a target the mask excludes.
 * Every output word is written exactly once, also for an empty profile, a profile holding every item or a query id outside [0, n_users);
 * nothing else is written, no workspace.  The result is a function of the input alone.  1 <= k <= arl_itemknn_max_k() = 128,
 * 1 <= n <= arl_itemknn_max_n() = 128, n_targets <= arl_itemknn_max_targets() = 64; tile_items = 0 takes arl_itemknn_default_tile_items()
 * (8 160 items = 64 KiB of 64-bit LDS accumulators, two workgroups per CU), at most arl_itemknn_max_tile_items() (18 400).  Negative sizes,
 * k < 1 or n < 1: ARL_E_ARG; k, n, n_targets, tile_items, n_users, n_items, n_queries, n_queries * n or n_queries * n_targets >= 2^31 past
 * their limits: ARL_E_RANGE; a NULL rowptr, idx or score, NULL neighbour lists with n_items > 0 or NULL target arguments with n_targets > 0,
 * with n_queries > 0: ARL_E_NULL; all before any launch.  Neighbour ids outside [0, n_items) are skipped. */
int64_t arl_itemknn_max_k(void);
int64_t arl_itemknn_max_n(void);
int64_t arl_itemknn_max_targets(void);
int64_t arl_itemknn_max_tile_items(void);
int64_t arl_itemknn_default_tile_items(void);
int arl_itemknn_score_topk_i64(const int64_t *rowptr, const int32_t *col, int64_t n_users, int64_t n_items, const int32_t *nbr_idx,
                               const int32_t *nbr_w, int64_t k, const int32_t *rows, int64_t n_queries, int64_t n, int32_t mask_profile,
                               const int32_t *tgt_id, const int32_t *tgt_col, int64_t n_targets, const int32_t *order, int64_t tile_items,
                               int32_t *idx, int64_t *score, int32_t *rank, arl_stream_t stream);

/* The user side of the same kernel (the scoring step of arlib_amd/recommender/UserKNN.py on the lists arl_cooccur_topk_i32 writes for the matrix
 * itself).  The argument list is arl_itemknn_score_topk_i64's with the lists indexed by user: nbr_idx, nbr_w [n_users, k] int32, neighbour
 * user r of user u and its non-negative weight, and
 *   s(u, i) = sum over r < k with v = nbr_idx[u, r] in [0, n_users) of nbr_w[u, r] [i in P_v],
 * taken as written: a neighbour named in two slots counts twice, a slot naming u itself counts.  Candidates, order, outputs, limits on k, n and
 * n_targets and the error codes are those above (NULL neighbour lists with n_users > 0: ARL_E_NULL); neighbour ids outside [0, n_users) are
 * skipped.  The fixed LDS grows by a cursor, an end and a weight per slot: tile_items = 0 takes arl_userknn_default_tile_items() (7 856 items,
 * 80 KiB in all, two workgroups per CU), at most arl_userknn_max_tile_items() (18 096). */
int64_t arl_userknn_max_tile_items(void);
int64_t arl_userknn_default_tile_items(void);
int arl_userknn_score_topk_i64(const int64_t *rowptr, const int32_t *col, int64_t n_users, int64_t n_items, const int32_t *nbr_idx,
                               const int32_t *nbr_w, int64_t k, const int32_t *rows, int64_t n_queries, int64_t n, int32_t mask_profile,
                               const int32_t *tgt_id, const int32_t *tgt_col, int64_t n_targets, const int32_t *order, int64_t tile_items,
                               int32_t *idx, int64_t *score, int32_t *rank, arl_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Item-table exchange of the user-sharded step (no reference counterpart: main.py:19 pins one device).
 * One process per GPU.  arl_comm_unique_id (rank 0) -> the 128 bytes travel to every rank by any side channel (torch.distributed
 * broadcast) -> arl_comm_init on every rank.  arl_allreduce_item_f32 sum-all-reduces buf[0, n_elems) IN PLACE, asynchronously on `stream`,
 * as a direct reduce-scatter + all-gather over the point-to-point xGMI links (every rank owns one shard, sums the P partials of it in rank
 * order -- deterministic, one writer per element -- and sends the result to every peer), cut into n_chunks chunks (1..64); workspace =
 * arl_allreduce_item_workspace_bytes(n_elems, world, n_chunks), 16-byte aligned like buf.  RCCL is bound at run time (dlopen of the
 * instance the process already has, or `rccl_path`); without it the arl_comm_* calls return ARL_E_ARG.  Returns 1000 + ncclResult_t on an
 * RCCL error.  arl_item_exchange_range: the [lo, hi) element range of chunk `chunk` of shard `shard` (host-side arithmetic, for tests).
 * ---------------------------------------------------------------------------------------------- */
typedef void *arl_comm_t;
int arl_comm_load(const char *rccl_path);
int arl_comm_unique_id(void *id128);
/* device: HIP device index the communicator binds to (made current for the call and restored); < 0 = the calling thread's current device */
int arl_comm_init(const void *id128, int64_t rank, int64_t world, int64_t device, arl_comm_t *out);
int arl_comm_destroy(arl_comm_t comm);
int arl_item_exchange_range(int64_t n_elems, int64_t world, int64_t n_chunks, int64_t shard, int64_t chunk, int64_t *lo, int64_t *hi);
int64_t arl_allreduce_item_workspace_bytes(int64_t n_elems, int64_t world, int64_t n_chunks);
int arl_allreduce_item_f32(arl_comm_t comm, float *buf, int64_t n_elems, int64_t n_chunks, void *workspace, arl_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ARLIB_AMD_H */

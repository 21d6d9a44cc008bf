"""Exact fixed-point user-kNN scoring with a full-catalogue top-N (the user side of csrc/arl_itemknn.hip; no reference counterpart): for a user u
with neighbour users nbr_idx[u, r] and weights nbr_w[u, r], s(u, i) = sum over r with v = nbr_idx[u, r] >= 0 of nbr_w[u, r] [i in P_v], the N
best items of the whole catalogue and the rank of given target items, without the n_users x n_items product.  A module of its own like
arlib_amd/itemknn.py, whose contract it shares word for word past the score; neighbours.cooccur_topk on the matrix itself writes the lists,
itemknn.knn_weights turns their integers into weights and itemknn.float_score forms the floats.  Its poisoned-memory sweep is
tests/test_gpu_userknn_poison.py.  DESIGN.md section 3u has the rules.

The sum is taken as written: a neighbour named in two slots counts twice and a slot naming u itself counts; cooccur_topk produces neither."""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import check
from .itemknn import KNN_MAX_N, KNN_MAX_TARGETS, ROUTES, _host_queries, _lists, _select, _validated, knn_supported
from .neighbours import _canonical, binary_csr

UKNN_MAX_TILE_ITEMS = 18096                                # arl_userknn_max_tile_items: 160 KiB of LDS minus the item side's fixed part and the slots' cursors
UKNN_DEFAULT_TILE_ITEMS = 7856                             # arl_userknn_default_tile_items: 80 KiB in all, two workgroups per CU
# route='auto' (tools/userknn_bench.py, profiles/userknn_bench.json): the kernel wherever its limits hold on a GPU, the host route
# past them or without a GPU


def _ops():
    from . import ops
    return ops


def uknn_supported(k, N, n_targets=0, n_users=0, n_items=0, n_queries=0):
    """True when the kernel takes the problem: itemknn.knn_supported's limits (1 <= k, N <= 128, at most 64 targets, sizes within int32)."""
    return knn_supported(k, N, n_targets, n_users, n_items, n_queries)


def uknn_score_topk(rowptr, col, n_users, n_items, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None, tile_items=None, device='cuda',
                    route='auto'):
    """(idx int32 [Q, N], score int64 [Q, N], rank int32 [Q, T] or None) for the binary n_users x n_items matrix X given as CSR (rowptr
    [n_users + 1], col [nnz]; tensors or arrays, any order within a row, repeated entries count once) and the user-side neighbour lists nbr_idx,
    nbr_w int32 [n_users, k] (nbr_idx[u, r] = -1: an unused slot, its weight ignored; weights non-negative).  Query q is user rows[q] (any order,
    repeats allowed), or user q when rows is None.  s(u, i) = sum over r with v = nbr_idx[u, r] >= 0 of nbr_w[u, r] [i in P_v], exact in int64
    and taken as written (a neighbour in two slots counts twice, a slot naming u counts).  Every item is a candidate, score 0 included; with
    mask_profile the items of P_u are not.  The order is (score descending, item id ascending).  idx[q] and score[q] hold the N best
    candidates, best first; unused slots are idx = -1, score = 0.  rank[q, t] is the number of candidates that beat targets[t] (distinct ids, at
    most 64), -1 when the mask excludes it; None without targets.

    route 'kernel' runs arl_userknn_score_topk_i64 on `device` (the rows are sorted and de-duplicated, the targets sorted and the launch order,
    heaviest query first by the summed degrees of its live neighbours, are built here with torch) and raises ValueError past uknn_supported;
    'host' is uknn_score_topk_host, its result as CPU tensors; 'auto' is the kernel where it is supported and the host route past its limits.
    The kernel needs a GPU: when the device is not one, 'auto' takes the host route and 'kernel' raises ValueError; nothing but device memory
    ever reaches the C entry.  ValueError for inconsistent shapes, a rowptr that does not rise from 0 to nnz, ids out of range (neighbour ids
    in [-1, n_users)), negative weights, repeated targets, N < 1, k < 1 or a tile_items outside [1, 18 096]: the kernel trusts what it is given."""
    who = 'uknn_score_topk'
    if route not in ROUTES:
        raise ValueError('%s: route %r, one of %s needed' % (who, route, ROUTES))
    host = route == 'host'
    dev = torch.device('cpu') if host else (rowptr.device if isinstance(rowptr, torch.Tensor) and rowptr.is_cuda else torch.device(device))
    if dev.type != 'cuda' and not host:
        if route == 'kernel':
            raise ValueError('%s: the kernel route needs a GPU, not device %r: use route=\'host\' or uknn_score_topk_host' % (who, str(dev)))
        host = True
    rp, ci, n_users, n_items, ni, nw, k, N, rw, tg = _validated(rowptr, col, n_users, n_items, nbr_idx, nbr_w, N, rows, targets, tile_items, dev, who,
                                                                UKNN_MAX_TILE_ITEMS, user_side=True)
    rp, ci, _, deg = _canonical(rp, ci, n_users, n_items)
    Q = n_users if rw is None else rw.numel()
    T = 0 if tg is None else tg.numel()
    if not host and not uknn_supported(k, N, T, n_users, n_items, Q):
        if route == 'kernel':
            raise ValueError('%s: k = %d, N = %d (at most %d), %d targets (at most %d), %d queries: use uknn_score_topk_host'
                             % (who, k, N, KNN_MAX_N, T, KNN_MAX_TARGETS, Q))
        host = True
    if host:
        X = sp.csr_matrix((np.ones(ci.numel(), np.int64), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n_users, n_items))
        hi, hs, hr = uknn_score_topk_host(X, ni.cpu().numpy(), nw.cpu().numpy(), N, None if rw is None else rw.cpu().numpy(), mask_profile,
                                          None if tg is None else tg.cpu().numpy())
        return torch.from_numpy(hi), torch.from_numpy(hs), None if hr is None else torch.from_numpy(hr)
    o = _ops()
    idx = torch.empty((Q, N), dtype=torch.int32, device=dev)
    score = torch.empty((Q, N), dtype=torch.int64, device=dev)
    rank = None if tg is None else torch.empty((Q, T), dtype=torch.int32, device=dev)
    if Q == 0:
        return idx, score, rank
    nq = ni if rw is None else ni[rw.long()]
    wq = torch.where(nq >= 0, deg[nq.clamp(min=0).long()], torch.zeros_like(nq, dtype=torch.int64)).sum(1)      # the entries the query's workgroup reads
    order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
    tid = tcol = None
    if T:
        srt = torch.sort(tg.long(), stable=True)
        tid, tcol = srt.values.to(torch.int32).contiguous(), srt.indices.to(torch.int32).contiguous()
    check(_lib.lib().arl_userknn_score_topk_i64(o._ptr(rp), o._ptr(ci), n_users, n_items, o._ptr(ni), o._ptr(nw), k, o._ptr(rw), Q, N,
                                                1 if mask_profile else 0, o._ptr(tid), o._ptr(tcol), T, o._ptr(order), int(tile_items or 0),
                                                o._ptr(idx), o._ptr(score), o._ptr(rank) if T else None, o._stream()), 'arl_userknn_score_topk_i64')
    return idx, score, rank


def weight_matrix(nbr_idx, nbr_w, n_users, rows=None):
    """The queried lists as the int64 sparse Q x n_users matrix W with W[q, v] = the summed weights of the slots of user rows[q] (user q when
    rows is None) that name v."""
    ni, nw = np.asarray(nbr_idx).astype(np.int64), np.asarray(nbr_w).astype(np.int64)
    if rows is not None:
        r = np.asarray(rows).astype(np.int64)
        ni, nw = ni[r], nw[r]
    used = ni >= 0
    q = np.broadcast_to(np.arange(ni.shape[0], dtype=np.int64)[:, None], ni.shape)[used]
    return sp.csr_matrix((nw[used], (q, ni[used])), shape=(ni.shape[0], n_users), dtype=np.int64)


def uknn_score_topk_host(interact, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None, chunk_rows=2048):
    """The contract of uknn_score_topk on the host, as numpy arrays (idx int32 [Q, N], score int64 [Q, N], rank int32 [Q, T] or None): scipy's
    product Wq @ X of Wq = weight_matrix of the queried lists with the binarised matrix (int64, exact), made dense chunk_rows query rows at a
    time, excluded items set to -1, and itemknn's selection (one lexsort on (id, -score) per chunk).  For CPU callers, for sizes past the
    kernel's limits and as the yardstick of the GPU tests; it holds chunk_rows x n_items int64 scores at a time."""
    who = 'uknn_score_topk_host'
    N = int(N)
    if N < 1:
        raise ValueError('%s: N = %d, N >= 1 needed' % (who, N))
    X = binary_csr(interact)
    n_users, n_items = X.shape
    ni, nw, _ = _lists(nbr_idx, nbr_w, n_users, torch.device('cpu'), who, 'n_users')
    ni, nw = ni.numpy(), nw.numpy()
    q_rows, tg = _host_queries(rows, targets, n_users, n_items, who)
    Q = len(q_rows)
    idx, score = np.full((Q, N), -1, np.int32), np.zeros((Q, N), np.int64)
    rank = None if tg is None else np.full((Q, len(tg)), -1, np.int32)
    for b in range(0, Q, max(int(chunk_rows), 1)):
        qr = q_rows[b:b + max(int(chunk_rows), 1)]
        S = np.asarray((weight_matrix(ni, nw, n_users, qr) @ X).todense(), dtype=np.int64)
        if mask_profile:
            Xq = X[qr]
            S[np.repeat(np.arange(len(qr)), np.diff(Xq.indptr)), Xq.indices] = -1
        _select(S, tg, idx[b:b + len(qr)], score[b:b + len(qr)], None if rank is None else rank[b:b + len(qr)])
    return idx, score, rank

"""Exact fixed-point item-kNN scoring with a full-catalogue top-N (csrc/arl_itemknn.hip; no reference counterpart): for a user u with profile P_u
and per-item neighbour lists (nbr_idx, nbr_w), s(u, i) = sum over j in P_u, r of [nbr_idx[j, r] == i] nbr_w[j, r], the N best items of the whole
catalogue and the rank of given target items, without the n_users x n_items product.  A module of its own like arlib_amd/neighbours.py, whose
cooccur_topk on the transposed matrix writes the lists; its poisoned-memory sweep is tests/test_gpu_itemknn_poison.py.  DESIGN.md section 3t has
the rules.

Integers decide, floats are formed afterwards in one place: the weights are non-negative int32 fixed-point numbers (knn_weights), the score is
their exact int64 sum, the order is (score descending, item id ascending), so the kernel, the host route and the pure-Python restatement of the
tests return the same integers.  The float score shown to users is score / 2^30 (SCALE) for the 'cosine' and 'jaccard' weights and the score
itself for 'count' (float_score)."""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import check
from .neighbours import MEASURES, _canonical, _measure, binary_csr

KNN_MAX_K = 128                                            # arl_itemknn_max_k
KNN_MAX_N = 128                                            # arl_itemknn_max_n
KNN_MAX_TARGETS = 64                                       # arl_itemknn_max_targets
KNN_MAX_TILE_ITEMS = 18400                                 # arl_itemknn_max_tile_items: 160 KiB of LDS minus the list, the pending buffer, the targets
KNN_DEFAULT_TILE_ITEMS = 8160                              # arl_itemknn_default_tile_items: 64 KiB of 64-bit accumulators, two workgroups per CU
SCALE = 2 ** 30                                            # a similarity of 1.0 as a weight
# route='auto' (tools/itemknn_bench.py, profiles/itemknn_bench.json): the kernel wherever its limits hold on a GPU -- it is ahead of
# the composed torch route at every measured shape -- and the host route past them or without a GPU
ROUTES = ('auto', 'kernel', 'host')


def _ops():
    from . import ops
    return ops


def knn_supported(k, N, n_targets=0, n_users=0, n_items=0, n_queries=0):
    """True when the kernel takes the problem: 1 <= k, N <= 128, at most 64 targets, sizes and both output sizes within int32."""
    return (1 <= int(k) <= KNN_MAX_K and 1 <= int(N) <= KNN_MAX_N and 0 <= int(n_targets) <= KNN_MAX_TARGETS
            and max(int(n_users), int(n_items), int(n_queries)) < 2 ** 31 and int(n_queries) * max(int(N), int(n_targets)) < 2 ** 31)


def knn_similarity(idx, cnt, deg, measure, shrink=0.0):
    """float64 [n_items, k] similarities from the integers of cooccur_topk / cooccur_topk_host run on all rows of the item x user matrix (row j of
    idx lists the neighbours of item j, deg the item degrees), formed the way neighbours.similarity forms them with `shrink` >= 0 added to the
    denominator: cnt ('count'), cnt / (sqrt(dj dv) + shrink) ('cosine'), cnt / (dj + dv - cnt + shrink) ('jaccard'); 0 in an unused slot."""
    _measure(measure)
    shrink = float(shrink)
    if not shrink >= 0.0:
        raise ValueError('knn_similarity: shrink = %r, shrink >= 0 needed' % shrink)
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    idx, cnt, deg = to_np(idx).astype(np.int64), to_np(cnt).astype(np.int64), to_np(deg).astype(np.int64)
    if idx.ndim != 2 or cnt.shape != idx.shape or deg.ndim != 1 or idx.shape[0] != deg.shape[0]:
        raise ValueError('knn_similarity: idx, cnt [n_items, k] and deg [n_items] needed')
    used = idx >= 0
    du = np.broadcast_to(deg[:, None], idx.shape)[used]
    dv, c = deg[idx[used]], cnt[used]
    out = np.zeros(idx.shape, np.float64)
    if measure == 'count':
        out[used] = c
    elif measure == 'cosine':
        out[used] = c / (np.sqrt((du * dv).astype(np.float64)) + shrink)
    else:
        out[used] = c / ((du + dv - c).astype(np.float64) + shrink)
    return out


def knn_weights(idx, cnt, deg, measure, shrink=0.0):
    """int32 [n_items, k] fixed-point weights from the same integers.  'count': cnt itself.  Otherwise w = floor(sim * 2^30) of knn_similarity's
    float64 sim: a similarity is at most 1, so w <= 2^30.  0 in an unused slot.  A host function.

    score / 2^30 is therefore the float score shown to users for 'cosine' and 'jaccard', and score itself for 'count' (float_score)."""
    sim = knn_similarity(idx, cnt, deg, measure, shrink)
    if measure == 'count':
        return sim.astype(np.int64).astype(np.int32)
    return np.floor(sim * SCALE).astype(np.int64).astype(np.int32)


def float_score(score, measure):
    """float64 scores from the int64 ones: score / 2^30 for the fixed-point measures, score for 'count'; formed here and nowhere else."""
    _measure(measure)
    s = score.detach().cpu().numpy() if isinstance(score, torch.Tensor) else np.asarray(score)
    return s.astype(np.float64) if measure == 'count' else s.astype(np.float64) / SCALE


def _lists(nbr_idx, nbr_w, n_items, dev, who, side='n_items'):
    """The neighbour lists as int32 [n_items, k] tensors on dev, checked: ids below n_items, weights of the used slots non-negative.  (The user
    side, arlib_amd/userknn.py, passes n_users and side='n_users'.)"""
    ni, nw = torch.as_tensor(nbr_idx).to(dev), torch.as_tensor(nbr_w).to(dev)
    if ni.dim() != 2 or nw.shape != ni.shape or ni.shape[0] != n_items or any(t.dtype.is_floating_point or t.dtype == torch.bool for t in (ni, nw)):
        raise ValueError('%s: integer nbr_idx and nbr_w of shape [%s = %d, k] needed' % (who, side, n_items))
    k = int(ni.shape[1])
    if k < 1:
        raise ValueError('%s: k = %d, k >= 1 needed' % (who, k))
    if ni.numel():
        if int(ni.max()) >= n_items or int(ni.min()) < -1:
            raise ValueError('%s: neighbour id outside [-1, %d)' % (who, n_items))
        used_w = torch.where(ni >= 0, nw, torch.zeros_like(nw))
        if int(used_w.min()) < 0 or int(used_w.max()) > 2 ** 31 - 1:
            raise ValueError('%s: weights must lie in [0, 2^31)' % who)
    return ni.to(torch.int32).contiguous(), nw.to(torch.int32).contiguous(), k   # after the range checks: a 64-bit value must not wrap into the range


def _validated(rowptr, col, n_users, n_items, nbr_idx, nbr_w, N, rows, targets, tile_items, dev, who='knn_score_topk', max_tile=KNN_MAX_TILE_ITEMS,
               user_side=False):
    n_users, n_items, N = int(n_users), int(n_items), int(N)
    if n_users < 0 or n_items < 0 or n_users >= 2 ** 31 or n_items >= 2 ** 31:
        raise ValueError('%s: n_users = %d, n_items = %d' % (who, n_users, n_items))
    if N < 1:
        raise ValueError('%s: N = %d, N >= 1 needed' % (who, N))
    if tile_items is not None and not 1 <= int(tile_items) <= max_tile:
        raise ValueError('%s: tile_items = %d outside [1, %d]' % (who, int(tile_items), max_tile))
    rp = torch.as_tensor(rowptr).to(dev, torch.int64).contiguous()
    ci = torch.as_tensor(col).to(dev)
    nnz = ci.numel()
    if rp.dim() != 1 or ci.dim() != 1 or rp.numel() != n_users + 1 or nnz >= 2 ** 31 or ci.dtype.is_floating_point or ci.dtype == torch.bool:
        raise ValueError('%s: rowptr [n_users + 1] and an integer col [nnz < 2^31] needed' % who)
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_users and int((rp[1:] - rp[:-1]).min()) < 0):
        raise ValueError('%s: rowptr must rise from 0 to nnz' % who)
    if nnz and (int(ci.min()) < 0 or int(ci.max()) >= n_items):
        raise ValueError('%s: item id outside [0, %d)' % (who, n_items))
    ci = ci.to(torch.int32).contiguous()
    ni, nw, k = _lists(nbr_idx, nbr_w, n_users, dev, who, 'n_users') if user_side else _lists(nbr_idx, nbr_w, n_items, dev, who)
    rw = None
    if rows is not None:
        rw = torch.as_tensor(rows).to(dev).contiguous()
        if rw.dim() != 1 or rw.dtype.is_floating_point or rw.dtype == torch.bool or rw.numel() >= 2 ** 31:
            raise ValueError('%s: rows must be a 1-d integer list' % who)
        if rw.numel() and (int(rw.min()) < 0 or int(rw.max()) >= n_users):
            raise ValueError('%s: query user outside [0, %d)' % (who, n_users))
        rw = rw.to(torch.int32)
    tg = None
    if targets is not None:
        tg = torch.as_tensor(targets).to(dev).contiguous()
        if tg.dim() != 1 or tg.dtype.is_floating_point or tg.dtype == torch.bool:
            raise ValueError('%s: targets must be a 1-d integer list' % who)
        if tg.numel() and (int(tg.min()) < 0 or int(tg.max()) >= n_items):
            raise ValueError('%s: target outside [0, %d)' % (who, n_items))
        if torch.unique(tg).numel() != tg.numel():
            raise ValueError('%s: repeated target' % who)
        tg = tg.to(torch.int32)
    return rp, ci, n_users, n_items, ni, nw, k, N, rw, tg


def knn_score_topk(rowptr, col, n_users, n_items, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None, tile_items=None, device='cuda',
                   route='auto'):
    """(idx int32 [Q, N], score int64 [Q, N], rank int32 [Q, T] or None) for the binary n_users x n_items matrix X given as CSR (rowptr
    [n_users + 1], col [nnz]; tensors or arrays, any order within a row, repeated entries count once) and the neighbour lists nbr_idx, nbr_w
    int32 [n_items, k] (nbr_idx[j, r] = -1: an unused slot, its weight ignored; weights non-negative).  Query q is user rows[q] (any order, repeats
    allowed), or user q when rows is None.  s(u, i) = sum over j in P_u, r of [nbr_idx[j, r] == i] nbr_w[j, r], exact in int64.  Every item is a
    candidate, score 0 included; with mask_profile the items of P_u are not.  The order is (score descending, item id ascending).  idx[q] and
    score[q] hold the N best candidates, best first; unused slots are idx = -1, score = 0.  rank[q, t] is the number of candidates that beat
    targets[t] (distinct ids, at most 64), -1 when the mask excludes it; None without targets.

    route 'kernel' runs arl_itemknn_score_topk_i64 on `device` (the rows are sorted and de-duplicated, the targets sorted and the launch order,
    heaviest query first by its live neighbour slots, are built here with torch) and raises ValueError past knn_supported; 'host' is
    knn_score_topk_host, its result as CPU tensors; 'auto' is the kernel where it is supported and the host route past its limits.  The kernel
    needs a GPU: when the device is not one, 'auto' takes the host route and 'kernel' raises ValueError; nothing but device memory ever reaches
    the C entry.  ValueError for inconsistent shapes, a rowptr that does not rise from 0 to nnz, ids out of range, negative weights, repeated
    targets, N < 1, k < 1 or a tile_items outside [1, 18 400]: the kernel trusts what it is given."""
    if route not in ROUTES:
        raise ValueError('knn_score_topk: route %r, one of %s needed' % (route, ROUTES))
    host = route == 'host'
    dev = torch.device('cpu') if host else (rowptr.device if isinstance(rowptr, torch.Tensor) and rowptr.is_cuda else torch.device(device))
    if dev.type != 'cuda' and not host:
        if route == 'kernel':
            raise ValueError('knn_score_topk: the kernel route needs a GPU, not device %r: use route=\'host\' or knn_score_topk_host' % str(dev))
        host = True
    rp, ci, n_users, n_items, ni, nw, k, N, rw, tg = _validated(rowptr, col, n_users, n_items, nbr_idx, nbr_w, N, rows, targets, tile_items, dev)
    rp, ci, r, _ = _canonical(rp, ci, n_users, n_items)
    Q = n_users if rw is None else rw.numel()
    T = 0 if tg is None else tg.numel()
    if not host and not knn_supported(k, N, T, n_users, n_items, Q):
        if route == 'kernel':
            raise ValueError('knn_score_topk: k = %d, N = %d (at most %d), %d targets (at most %d), %d queries: use knn_score_topk_host'
                             % (k, N, KNN_MAX_N, T, KNN_MAX_TARGETS, Q))
        host = True
    if host:
        X = sp.csr_matrix((np.ones(ci.numel(), np.int64), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n_users, n_items))
        hi, hs, hr = knn_score_topk_host(X, ni.cpu().numpy(), nw.cpu().numpy(), N, None if rw is None else rw.cpu().numpy(), mask_profile,
                                         None if tg is None else tg.cpu().numpy())
        return torch.from_numpy(hi), torch.from_numpy(hs), None if hr is None else torch.from_numpy(hr)
    o = _ops()
    idx = torch.empty((Q, N), dtype=torch.int32, device=dev)
    score = torch.empty((Q, N), dtype=torch.int64, device=dev)
    rank = None if tg is None else torch.empty((Q, T), dtype=torch.int32, device=dev)
    if Q == 0:
        return idx, score, rank
    live = (ni >= 0).sum(1)
    weight = torch.zeros(n_users, dtype=torch.int64, device=dev).index_add_(0, r, live[ci.long()])
    wq = weight if rw is None else weight[rw.long()]
    order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
    tid = tcol = None
    if T:
        srt = torch.sort(tg.long(), stable=True)
        tid, tcol = srt.values.to(torch.int32).contiguous(), srt.indices.to(torch.int32).contiguous()
    check(_lib.lib().arl_itemknn_score_topk_i64(o._ptr(rp), o._ptr(ci), n_users, n_items, o._ptr(ni), o._ptr(nw), k, o._ptr(rw), Q, N,
                                                1 if mask_profile else 0, o._ptr(tid), o._ptr(tcol), T, o._ptr(order), int(tile_items or 0),
                                                o._ptr(idx), o._ptr(score), o._ptr(rank) if T else None, o._stream()), 'arl_itemknn_score_topk_i64')
    return idx, score, rank


def weight_matrix(nbr_idx, nbr_w, n_items):
    """The lists as the int64 sparse n_items x n_items matrix W with W[j, i] = the summed weights of item j's slots that name i."""
    ni, nw = np.asarray(nbr_idx).astype(np.int64), np.asarray(nbr_w).astype(np.int64)
    used = ni >= 0
    j = np.broadcast_to(np.arange(ni.shape[0], dtype=np.int64)[:, None], ni.shape)[used]
    return sp.csr_matrix((nw[used], (j, ni[used])), shape=(n_items, n_items), dtype=np.int64)


def _host_queries(rows, targets, n_users, n_items, who):
    """(query users int64 [Q], targets int64 [T] or None) of a host route, checked."""
    if rows is None:
        q_rows = np.arange(n_users, dtype=np.int64)
    else:
        q_rows = np.asarray(rows)
        if q_rows.ndim != 1 or q_rows.dtype.kind not in 'iu' or (q_rows.size and (q_rows.min() < 0 or q_rows.max() >= n_users)):
            raise ValueError('%s: rows must be a 1-d list of ids in [0, %d)' % (who, n_users))
        q_rows = q_rows.astype(np.int64)
    tg = None
    if targets is not None:
        tg = np.asarray(targets)
        if tg.ndim != 1 or (tg.size and tg.dtype.kind not in 'iu') or (tg.size and (tg.min() < 0 or tg.max() >= n_items)) or len(np.unique(tg)) != len(tg):
            raise ValueError('%s: targets must be distinct ids in [0, %d)' % (who, n_items))
        tg = tg.astype(np.int64)
    return q_rows, tg


def _select(S, tg, idx, score, rank):
    """The selection of both host routes (this module's and arlib_amd/userknn.py's) on a dense chunk S int64 [q, n_items] of scores with the
    excluded items set to -1: one lexsort on (id, -score) fills idx, score [q, N] (preset to -1, 0), and the candidates that beat each target
    are counted into rank [q, T] (preset to -1)."""
    q, n_items = S.shape
    m = min(idx.shape[1], n_items)
    n_cand = (S >= 0).sum(1)
    if m:
        ids = np.arange(n_items, dtype=np.int64)
        p = np.lexsort((np.broadcast_to(ids, S.shape).ravel(), -S.ravel(), np.repeat(np.arange(q), n_items)))
        top = (p.reshape(q, n_items)[:, :m] % n_items).astype(np.int64)
        ts = np.take_along_axis(S, top, 1)
        ok = np.arange(m)[None, :] < n_cand[:, None]
        idx[:, :m] = np.where(ok, top, -1)
        score[:, :m] = np.where(ok, ts, 0)
    if tg is not None:
        for t, item in enumerate(tg.tolist()):
            st = S[:, item]
            beat = ((S > st[:, None]) & (S >= 0)).sum(1) + (S[:, :item] == st[:, None]).sum(1)
            rank[:, t] = np.where(st >= 0, beat, -1)


def knn_score_topk_host(interact, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None, chunk_rows=2048):
    """The contract of knn_score_topk on the host, as numpy arrays (idx int32 [Q, N], score int64 [Q, N], rank int32 [Q, T] or None): scipy's
    product X[rows] @ W of the binarised matrix with W = weight_matrix (int64, exact), made dense chunk_rows query rows at a time, excluded
    items set to -1, and one lexsort on (id, -score) per chunk.  For CPU callers, for sizes past the kernel's limits and as the yardstick of the
    GPU tests; it holds chunk_rows x n_items int64 scores at a time."""
    N = int(N)
    if N < 1:
        raise ValueError('knn_score_topk_host: N = %d, N >= 1 needed' % N)
    X = binary_csr(interact)
    n_users, n_items = X.shape
    ni, nw, _ = _lists(nbr_idx, nbr_w, n_items, torch.device('cpu'), 'knn_score_topk_host')
    W = weight_matrix(ni.numpy(), nw.numpy(), n_items)
    q_rows, tg = _host_queries(rows, targets, n_users, n_items, 'knn_score_topk_host')
    Q = len(q_rows)
    idx, score = np.full((Q, N), -1, np.int32), np.zeros((Q, N), np.int64)
    rank = None if tg is None else np.full((Q, len(tg)), -1, np.int32)
    for b in range(0, Q, max(int(chunk_rows), 1)):
        qr = q_rows[b:b + max(int(chunk_rows), 1)]
        Xq = X[qr]
        S = np.asarray((Xq @ W).todense(), dtype=np.int64)
        if mask_profile:
            S[np.repeat(np.arange(len(qr)), np.diff(Xq.indptr)), Xq.indices] = -1
        _select(S, tg, idx[b:b + len(qr)], score[b:b + len(qr)], None if rank is None else rank[b:b + len(qr)])
    return idx, score, rank

"""Exact top-k co-occurrence neighbours of the rows of a sparse binary matrix (csrc/arl_cooccur.hip; no reference counterpart): for a row u the
k other rows v with the largest similarity among those with c(u, v) = |X_u & X_v| > 0, without the n_rows x n_rows product.  A module of its
own like arlib_amd/corating.py, with its poisoned-memory sweep in tests/test_gpu_cooccur_poison.py.  DESIGN.md section 3s has the rules.

The order is decided in integers (count: c; cosine: c1^2 d2 against c2^2 d1; Jaccard: c1 (du + d2 - c2) against c2 (du + d1 - c1); ties to the
smaller row id), so the kernel, the host route and the pure-Python restatement of the tests return the same integers, and `similarity` turns them
into float64 on the host in one place: a similarity obtained through the kernel equals one obtained through the host route bit for bit."""
import functools

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import check

MEASURES = {'count': 0, 'cosine': 1, 'jaccard': 2}
COOCCUR_MAX_K = 128                                        # arl_cooccur_max_k
COOCCUR_MAX_TILE_ROWS = 36864                              # arl_cooccur_max_tile_rows: 160 KiB of LDS minus the list, the pending buffer, the cursors
COOCCUR_DEFAULT_TILE_ROWS = 16384                          # arl_cooccur_default_tile_rows: 64 KiB of counters, two workgroups per CU
COOCCUR_MAX_DEGREE = {'count': 2 ** 31 - 1, 'cosine': 2 ** 20, 'jaccard': 2 ** 31 - 1}     # arl_cooccur_max_degree: 64-bit keys cannot overflow
# route='auto' (tools/cooccur_bench.py, profiles/cooccur_bench.json): the kernel wherever its limits hold; the host route past them
ROUTES = ('auto', 'kernel', 'host')


def _ops():
    from . import ops
    return ops


def _measure(measure):
    if measure not in MEASURES:
        raise ValueError('cooccur_topk: measure %r, one of %s needed' % (measure, sorted(MEASURES)))
    return MEASURES[measure]


def cooccur_supported(k, measure, max_degree, n_rows=0, n_cols=0, n_queries=0):
    """True when the kernel takes the problem: 1 <= k <= 128, every degree within the bound of the measure's 64-bit keys, sizes within int32."""
    return (1 <= int(k) <= COOCCUR_MAX_K and 0 <= int(max_degree) <= COOCCUR_MAX_DEGREE[measure] and max(int(n_rows), int(n_cols), int(n_queries)) < 2 ** 31
            and int(n_queries) * int(k) < 2 ** 31)


def _canonical(rp, ci, n_rows, n_cols):
    """(rowptr, col, r, deg) with every row sorted and without repeats, on the device of rp: r [nnz] is the row of every kept entry."""
    deg = rp[1:] - rp[:-1]
    r = torch.repeat_interleave(torch.arange(n_rows, device=rp.device), deg)
    key = torch.unique(r * max(n_cols, 1) + ci.long(), sorted=True)
    r, c = torch.div(key, max(n_cols, 1), rounding_mode='floor'), key % max(n_cols, 1)
    deg = torch.bincount(r, minlength=n_rows)
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rp.device)
    rowptr[1:] = torch.cumsum(deg, 0)
    return rowptr, c.to(torch.int32).contiguous(), r, deg


def _col_major(r, c, n_rows, n_cols):
    """(colptr int64 [n_cols + 1], irow int32 [nnz], weight int64 [n_rows]) of canonical entries (r, c) sorted by (row, column): rows ascend within
    a column because the sort is stable; weight[u] = the summed degrees of u's columns, the counter increments u's workgroup issues."""
    cl = c.long()
    irow = r[torch.sort(cl, stable=True).indices].to(torch.int32).contiguous()
    cdeg = torch.bincount(cl, minlength=n_cols)
    colptr = torch.zeros(n_cols + 1, dtype=torch.int64, device=r.device)
    colptr[1:] = torch.cumsum(cdeg, 0)
    weight = torch.zeros(n_rows, dtype=torch.int64, device=r.device).index_add_(0, r, cdeg[cl])
    return colptr, irow, weight


def _validated(rowptr, col, n_rows, n_cols, k, measure, rows, tile_rows, dev):
    n_rows, n_cols, k = int(n_rows), int(n_cols), int(k)
    _measure(measure)
    if n_rows < 0 or n_cols < 0 or n_rows >= 2 ** 31 or n_cols >= 2 ** 31:
        raise ValueError('cooccur_topk: n_rows = %d, n_cols = %d' % (n_rows, n_cols))
    if k < 1:
        raise ValueError('cooccur_topk: k = %d, k >= 1 needed' % k)
    if tile_rows is not None and not 1 <= int(tile_rows) <= COOCCUR_MAX_TILE_ROWS:
        raise ValueError('cooccur_topk: tile_rows = %d outside [1, %d]' % (int(tile_rows), COOCCUR_MAX_TILE_ROWS))
    rp = torch.as_tensor(rowptr).to(dev, torch.int64).contiguous()
    ci = torch.as_tensor(col).to(dev)
    nnz = ci.numel()
    if rp.dim() != 1 or ci.dim() != 1 or rp.numel() != n_rows + 1 or nnz >= 2 ** 31 or ci.dtype.is_floating_point or ci.dtype == torch.bool:
        raise ValueError('cooccur_topk: rowptr [n_rows + 1] and an integer col [nnz < 2^31] needed')
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_rows and int((rp[1:] - rp[:-1]).min()) < 0):
        raise ValueError('cooccur_topk: rowptr must rise from 0 to nnz')
    if nnz and (int(ci.min()) < 0 or int(ci.max()) >= n_cols):
        raise ValueError('cooccur_topk: column id outside [0, %d)' % n_cols)
    ci = ci.to(torch.int32).contiguous()                     # after the range check: a 64-bit id must not wrap into the range
    rw = None
    if rows is not None:
        rw = torch.as_tensor(rows).to(dev).contiguous()
        if rw.dim() != 1 or rw.dtype.is_floating_point or rw.dtype == torch.bool or rw.numel() >= 2 ** 31:
            raise ValueError('cooccur_topk: rows must be a 1-d integer list')
        if rw.numel() and (int(rw.min()) < 0 or int(rw.max()) >= n_rows):
            raise ValueError('cooccur_topk: query row outside [0, %d)' % n_rows)
        rw = rw.to(torch.int32)
    return rp, ci, n_rows, n_cols, k, rw


def cooccur_topk(rowptr, col, n_rows, n_cols, k, measure='cosine', rows=None, tile_rows=None, device='cuda', route='auto'):
    """(idx int32 [Q, k], cnt int32 [Q, k], deg int64 [n_rows]) for the binary n_rows x n_cols matrix X given as CSR (rowptr [n_rows + 1],
    col [nnz]; tensors or arrays, any order within a row, repeated entries count once).  Query q is row rows[q] (any order, repeats allowed), or
    row q when rows is None.  idx[q] lists up to k rows v != u with c = |X_u & X_v| > 0, best first by `measure` ('count': c, 'cosine':
    c / sqrt(du dv), 'jaccard': c / (du + dv - c)), ties to the smaller row id; cnt holds c; unused slots are idx = -1, cnt = 0.  deg is the
    row degree after the repeats are removed.

    route 'kernel' runs arl_cooccur_topk_i32 on `device` (the rows are sorted and de-duplicated, the column-major index and the launch order,
    heaviest query first, are built here with torch) and raises ValueError past cooccur_supported; 'host' is cooccur_topk_host, its result
    as CPU tensors; 'auto' is the kernel where it is supported and the host route past its limits.  The kernel needs a GPU: when the device is
    not one, 'auto' takes the host route and 'kernel' raises ValueError; nothing but device memory ever reaches the C entry.  ValueError for inconsistent shapes, a
    rowptr that does not rise from 0 to nnz, ids out of range, k < 1 or a tile_rows outside [1, 36 864]: the kernel trusts what it is given."""
    if route not in ROUTES:
        raise ValueError('cooccur_topk: route %r, one of %s needed' % (route, ROUTES))
    host = route == 'host'
    dev = torch.device('cpu') if host else (rowptr.device if isinstance(rowptr, torch.Tensor) and rowptr.is_cuda else torch.device(device))
    if dev.type != 'cuda' and not host:
        if route == 'kernel':
            raise ValueError('cooccur_topk: the kernel route needs a GPU, not device %r: use route=\'host\' or cooccur_topk_host' % str(dev))
        host = True
    rp, ci, n_rows, n_cols, k, rw = _validated(rowptr, col, n_rows, n_cols, k, measure, rows, tile_rows, dev)
    rp, ci, r, deg = _canonical(rp, ci, n_rows, n_cols)
    Q = n_rows if rw is None else rw.numel()
    max_deg = int(deg.max()) if n_rows else 0
    if not host and not cooccur_supported(k, measure, max_deg, n_rows, n_cols, Q):
        if route == 'kernel':
            raise ValueError('cooccur_topk: k = %d (at most %d), largest degree %d (at most %d for %s), %d queries: use cooccur_topk_host'
                             % (k, COOCCUR_MAX_K, max_deg, COOCCUR_MAX_DEGREE[measure], measure, Q))
        host = True
    if host:
        X = sp.csr_matrix((np.ones(ci.numel(), np.int64), ci.cpu().numpy(), rp.cpu().numpy()), shape=(n_rows, n_cols))
        hi, hc, hd = cooccur_topk_host(X, k, measure, None if rw is None else rw.cpu().numpy())
        return torch.from_numpy(hi), torch.from_numpy(hc), torch.from_numpy(hd)
    o = _ops()
    idx = torch.empty((Q, k), dtype=torch.int32, device=dev)
    cnt = torch.empty((Q, k), dtype=torch.int32, device=dev)
    if Q == 0:
        return idx, cnt, deg
    colptr, irow, weight = _col_major(r, ci, n_rows, n_cols)
    wq = weight if rw is None else weight[rw.long()]
    order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
    check(_lib.lib().arl_cooccur_topk_i32(o._ptr(rp), o._ptr(ci), o._ptr(colptr), o._ptr(irow), n_rows, n_cols, o._ptr(rw), Q, k, MEASURES[measure],
                                          max_deg, o._ptr(order), int(tile_rows or 0), o._ptr(idx), o._ptr(cnt), o._stream()), 'arl_cooccur_topk_i32')
    return idx, cnt, deg


def binary_csr(interact):
    """The int64 CSR matrix with a 1 wherever `interact` stores a nonzero value, repeats merged, columns ascending within a row."""
    X = sp.csr_matrix(interact, copy=True)
    X.sum_duplicates()
    X.eliminate_zeros()
    X.sort_indices()
    return sp.csr_matrix((np.ones(len(X.data), np.int64), X.indices, X.indptr), shape=X.shape)


def _beats_py(measure, du):
    """The order as a comparison of (c, d, id) triples of Python ints: negative when a comes first."""
    def cmp(a, b):
        if measure == 'count':
            ka, kb = a[0], b[0]
        elif measure == 'cosine':
            ka, kb = a[0] * a[0] * b[1], b[0] * b[0] * a[1]
        else:
            ka, kb = a[0] * (du + b[1] - b[0]), b[0] * (du + a[1] - a[0])
        return -1 if ka > kb or (ka == kb and a[2] < b[2]) else (1 if (ka, a[2]) != (kb, b[2]) else 0)
    return cmp


def cooccur_topk_host(interact, k, measure='cosine', rows=None):
    """The contract of cooccur_topk on the host, as numpy arrays (idx int32 [Q, k], cnt int32 [Q, k], deg int64 [n_rows]): the scipy product
    X[rows] @ X.T of the binarised matrix, integer keys, ties to the smaller id.  Candidates are pre-sorted by a float64 key and every adjacent
    pair of the result is then checked with the exact int64 cross-multiplied comparison (a sequence is sorted by a strict total order exactly
    when each adjacent pair is); a query where that check fails, and every query when a degree is past the int64 bound of the measure, is
    sorted with Python ints.  For CPU callers, for sizes past the kernel's limits and as the yardstick of the GPU tests; scipy holds Q x n_rows
    counts in sparse form, so it ends where those no longer fit."""
    _measure(measure)
    k = int(k)
    if k < 1:
        raise ValueError('cooccur_topk_host: k = %d, k >= 1 needed' % k)
    X = binary_csr(interact)
    n_rows = X.shape[0]
    deg = np.diff(X.indptr).astype(np.int64)
    if rows is None:
        q_rows = np.arange(n_rows, dtype=np.int64)
    else:
        q_rows = np.asarray(rows)
        if q_rows.ndim != 1 or q_rows.dtype.kind not in 'iu' or (q_rows.size and (q_rows.min() < 0 or q_rows.max() >= n_rows)):
            raise ValueError('cooccur_topk_host: rows must be a 1-d list of ids in [0, %d)' % n_rows)
        q_rows = q_rows.astype(np.int64)
    Q = len(q_rows)
    idx, cnt = np.full((Q, k), -1, np.int32), np.zeros((Q, k), np.int32)
    if Q == 0 or X.nnz == 0:
        return idx, cnt, deg
    C = (X[q_rows] @ X.T).tocsr()
    qs = np.repeat(np.arange(Q, dtype=np.int64), np.diff(C.indptr))
    v, c = C.indices.astype(np.int64), C.data.astype(np.int64)
    keep = (c > 0) & (v != q_rows[qs])
    qs, v, c = qs[keep], v[keep], c[keep]
    d, du = deg[v], deg[q_rows[qs]]
    if measure == 'count':
        f = c.astype(np.float64)
    elif measure == 'cosine':
        f = (c * c).astype(np.float64) / d
    else:
        f = c / (du + d - c).astype(np.float64)
    p = np.lexsort((v, -f, qs))
    qs, v, c, d, du = qs[p], v[p], c[p], d[p], du[p]
    exact64 = int(deg.max()) <= (2 ** 20 if measure == 'cosine' else 2 ** 31 - 1)
    same = qs[1:] == qs[:-1]
    if exact64:
        if measure == 'count':
            ka, kb = c[:-1], c[1:]
        elif measure == 'cosine':
            ka, kb = c[:-1] * c[:-1] * d[1:], c[1:] * c[1:] * d[:-1]
        else:
            ka, kb = c[:-1] * (du[:-1] + d[1:] - c[1:]), c[1:] * (du[:-1] + d[:-1] - c[:-1])
        bad = np.unique(qs[1:][same & ~((ka > kb) | ((ka == kb) & (v[:-1] < v[1:])))])
    else:
        bad = np.unique(qs)
    start = np.searchsorted(qs, np.arange(Q + 1))
    pos = np.arange(len(qs)) - start[qs]
    top = pos < k
    idx[qs[top], pos[top]], cnt[qs[top], pos[top]] = v[top], c[top]
    for q in bad:                                           # exact, with Python ints
        s, e = start[q], start[q + 1]
        tri = sorted(zip(c[s:e].tolist(), d[s:e].tolist(), v[s:e].tolist()), key=functools.cmp_to_key(_beats_py(measure, int(deg[q_rows[q]]))))[:k]
        idx[q], cnt[q] = -1, 0
        idx[q, :len(tri)], cnt[q, :len(tri)] = [t[2] for t in tri], [t[0] for t in tri]
    return idx, cnt, deg


def similarity(idx, cnt, deg, rows=None, measure='cosine'):
    """float64 [Q, k] similarities from the integers of cooccur_topk / cooccur_topk_host, computed on the host: cnt ('count'),
    cnt / sqrt(du dv) ('cosine': du dv < 2^62 is formed in int64 and rounded once), cnt / (du + dv - cnt) ('jaccard'); 0 in an unused slot.
    rows is the query list the integers were computed with (None: all rows)."""
    _measure(measure)
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    idx, cnt, deg = to_np(idx).astype(np.int64), to_np(cnt).astype(np.int64), to_np(deg).astype(np.int64)
    q_rows = np.arange(idx.shape[0]) if rows is None else to_np(rows).astype(np.int64)
    used = idx >= 0
    du = np.broadcast_to(deg[q_rows][:, None], idx.shape)[used]
    dv, c = deg[idx[used]], cnt[used]
    out = np.zeros(idx.shape, np.float64)
    if measure == 'count':
        out[used] = c
    elif measure == 'cosine':
        out[used] = c / np.sqrt((du * dv).astype(np.float64))
    else:
        out[used] = c / (du + dv - c).astype(np.float64)
    return out

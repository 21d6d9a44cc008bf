"""Lloyd's k-means on the device (csrc/arl_kmeans.hip; reference recommender/NCL.py:52-73, e_step / run_kmeans) as tensor-level ops: the assign
and update passes, the random-rows start (the k-means++ start lives in arlib_amd/seeding.py), and the loop.  NCL's opt-in `kmeans = 'device'` back
end; a module of its own like arlib_amd/colsoftmax.py, with its poisoned-memory sweep in tests/test_gpu_kmeans_poison.py.  DESIGN.md section 3g
has the rules."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check

KMEANS_WIDTHS = ops.NCE_ALLROWS_WIDTHS
KMEANS_MAX_ROWS = (2 ** 31 - 1) // 128          # rows of either table: every row * d offset of the kernels' index arithmetic stays in int32


def _table(t, name, what):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError('%s: %s must be a 2-d torch.Tensor' % (what, name))
    if t.shape[1] not in KMEANS_WIDTHS:
        raise ValueError('%s: width %d outside %s' % (what, t.shape[1], KMEANS_WIDTHS))
    if t.dtype != torch.float32:
        raise ValueError('%s: %s must be float32, got %s' % (what, name, t.dtype))
    if not t.is_cuda:
        raise ValueError('%s: %s must be on the GPU (there is no host route), got %s' % (what, name, t.device))
    if not 1 <= t.shape[0] <= KMEANS_MAX_ROWS:
        raise ValueError('%s: %s needs 1 <= rows <= %d' % (what, name, KMEANS_MAX_ROWS))
    return t.contiguous()


def kmeans_assign(X, C):
    """labels int32 [N], score float32 [N]: labels[n] = argmax_c (<x_n, c> - |c|^2 / 2), the nearest centroid of C [k, d] to row n of X [N, d], and
    that maximum (|x_n - c|^2 = |x_n|^2 - 2 score[n]).  Equal scores go to the lower index; a row whose scores are all NaN gets label 0."""
    X, C = _table(X, 'X', 'kmeans_assign'), _table(C, 'C', 'kmeans_assign')
    if X.shape[1] != C.shape[1] or X.device != C.device:
        raise ValueError('kmeans_assign: X [N, d] and C [k, d] on one device')
    (N, d), k = X.shape, C.shape[0]
    bias = torch.empty(k, dtype=torch.float32, device=X.device)
    labels, score = torch.empty(N, dtype=torch.int32, device=X.device), torch.empty(N, dtype=torch.float32, device=X.device)
    check(_lib.lib().arl_kmeans_assign_f32(ops._ptr(X), N, ops._ptr(C), k, d, ops._ptr(bias), ops._ptr(labels), ops._ptr(score), ops._stream()),
          'arl_kmeans_assign_f32')
    return labels, score


def kmeans_update(X, labels, C_prev, check_range=True):
    """C_new float32 [k, d], counts int64 [k]: C_new[c] = the mean of the rows of X labelled c (summed in ascending row order, in fixed chunks),
    C_prev[c] bit for bit where no row is.  labels: integer [N] in [0, k) (check_range=False skips the host read that verifies it: for labels
    that kmeans_assign produced)."""
    X, C_prev = _table(X, 'X', 'kmeans_update'), _table(C_prev, 'C_prev', 'kmeans_update')
    (N, d), k = X.shape, C_prev.shape[0]
    if not isinstance(labels, torch.Tensor) or labels.dtype not in (torch.int32, torch.int64) or labels.shape != (N,) or labels.device != X.device \
            or C_prev.shape[1] != d or C_prev.device != X.device:
        raise ValueError('kmeans_update: X [N, d], integer labels [N] and C_prev [k, d] on one device')
    if check_range and (int(labels.min()) < 0 or int(labels.max()) >= k):
        raise ValueError('kmeans_update: labels outside [0, %d)' % k)
    L = _lib.lib()
    chunk = L.arl_kmeans_chunk_rows()
    by_label, order = torch.sort(labels, stable=True)                        # member rows of cluster 0 ascending, then cluster 1, ...
    # first position of every cluster in the sorted list (no host read; a label outside [0, k) falls outside every segment and is ignored)
    seg = torch.searchsorted(by_label, torch.arange(k + 1, dtype=labels.dtype, device=X.device))
    counts = seg[1:] - seg[:-1]
    chunk_ptr = torch.zeros(k + 1, dtype=torch.int32, device=X.device)
    chunk_ptr[1:] = torch.cumsum((counts + (chunk - 1)) // chunk, 0)
    order, seg_ptr = order.to(torch.int32), seg.to(torch.int32)
    ws = torch.empty(max(L.arl_kmeans_update_workspace_bytes(N, k, d), 16), dtype=torch.uint8, device=X.device)
    C_new = torch.empty_like(C_prev)
    check(L.arl_kmeans_update_f32(ops._ptr(X), N, d, ops._ptr(order), ops._ptr(seg_ptr), ops._ptr(chunk_ptr), k, ops._ptr(C_prev), ops._ptr(C_new), ops._ptr(ws),
                                  ops._stream()), 'arl_kmeans_update_f32')
    return C_new, counts


def _sum_f64(v, squared):
    L = _lib.lib()
    ws = torch.empty(L.arl_kmeans_sum_workspace_bytes() // 8, dtype=torch.float64, device=v.device)
    out = torch.empty(1, dtype=torch.float64, device=v.device)
    check(L.arl_kmeans_sum_f64(ops._ptr(v), v.numel(), 1 if squared else 0, ops._ptr(out), ops._ptr(ws), ops._stream()), 'arl_kmeans_sum_f64')
    return out


def kmeans_init_indices(N, k):
    """The k distinct start rows: exactly numpy.random.choice(N, size=k, replace=False) on numpy's GLOBAL generator -- the one sklearn's KMeans draws
    from with random_state=None (the reference's call) and util.tool.seedSet seeds, so a seeded run stays a seeded run."""
    return np.random.choice(int(N), size=int(k), replace=False)


def kmeans(X, k, n_iter=20, init=None):
    """Lloyd's k-means of the rows of X [N, d] (float32, on the GPU) into k clusters.  Start: `init` [k, d], or 'k-means++' for
    X[seeding.kmeanspp(X, k)] (sklearn's greedy k-means++ on the device), else X[kmeans_init_indices(N, k)].
    Every pass assigns (kmeans_assign) and, unless the pass changed no label (one integer read back per pass) or n_iter updates are done, updates
    (kmeans_update); the last pass is an assign against the final centroids, so labels and centroids agree (as kmeans.predict(x), NCL.py:73).
    Returns (centroids float32 [k, d], labels int64 [N], inertia: list with one float per assign pass, number of updates run).  An empty cluster
    keeps its centroid.  ValueError for N < k, k < 1, an unsupported width, a host or non-float32 table: there is no other route."""
    k, n_iter = int(k), int(n_iter)
    if k < 1:
        raise ValueError('kmeans: k = %d, at least one cluster needed' % k)
    if n_iter < 0:
        raise ValueError('kmeans: n_iter = %d' % n_iter)
    if isinstance(init, str) and init != 'k-means++':
        raise ValueError("kmeans: init must be None, 'k-means++' or a [k, d] tensor, got %r" % (init,))
    if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[0] < k:
        raise ValueError('kmeans: n_samples=%d should be >= n_clusters=%d' % (X.shape[0], k))
    X = _table(X, 'X', 'kmeans')
    N, d = X.shape
    if init is None:
        C = X[torch.from_numpy(kmeans_init_indices(N, k).astype(np.int64)).to(X.device)]
    elif isinstance(init, str):
        from . import seeding
        C = X[seeding.kmeanspp(X, k)]
    else:
        C = _table(init, 'init', 'kmeans')
        if C.shape != (k, d) or C.device != X.device:
            raise ValueError('kmeans: init must be [k, d] = [%d, %d] on the device of X' % (k, d))
    xsq = _sum_f64(X, True)
    inertia, prev, done = [], None, 0
    while True:
        labels, score = kmeans_assign(X, C)
        inertia.append(xsq - 2.0 * _sum_f64(score, False))
        if (prev is not None and int(torch.count_nonzero(labels != prev)) == 0) or done == n_iter:
            break
        C, _ = kmeans_update(X, labels, C, check_range=False)
        prev, done = labels, done + 1
    return C, labels.to(torch.int64), torch.cat(inertia).tolist(), done

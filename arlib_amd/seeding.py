"""Greedy k-means++ on the device (csrc/arl_kmeans.hip: kpp_dist_kernel, kpp_pick_kernel): the start sklearn's KMeans gives Lloyd's iteration
(sklearn.cluster._kmeans._kmeans_plusplus with unit sample weights), offered to arlib_amd/cluster.py as `init='k-means++'`.  The draws come from
numpy's global generator on the host, in sklearn's order, before anything is enqueued; the k - 1 steps then run without a host read.  A module of
its own like arlib_amd/cluster.py, with its poisoned-memory sweep in tests/test_gpu_kmeanspp_poison.py.  DESIGN.md section 3g has the rules."""
import numpy as np
import torch

from . import _lib, ops
from ._lib import check
from .cluster import _table

KMEANSPP_MAX_TRIALS = 16


def _n_trials(k):
    return 2 + int(np.log(k))                   # sklearn's n_local_trials


def kmeanspp_draws(N, k):
    """(first, u): the first centre's row and the uniforms float64 [k - 1, T], T = 2 + floor(ln k), of the k - 1 greedy steps: exactly sklearn's
    draws with unit weights on numpy's GLOBAL generator (random_state.choice(N, p=1/N), then uniform(size=T) per step), which util.tool.seedSet
    seeds: a seeded run stays a seeded run and the generator is left where these draws leave it."""
    N, k = int(N), int(k)
    first = int(np.random.choice(N, p=np.full(N, 1.0 / N)))
    return first, np.random.uniform(size=(k - 1, _n_trials(k)))


def _ids(t, name, what, device):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not 1 <= t.shape[0] <= KMEANSPP_MAX_TRIALS or t.device != device:
        raise ValueError('%s: %s must be int32 [T], 1 <= T <= %d, on the device of the table' % (what, name, KMEANSPP_MAX_TRIALS))
    return t.contiguous()


def kmeanspp_dist(X, cand_ids, closest=None):
    """One distance pass: mins float32 [T, N], mins[t, n] = min(closest[n], |x_n - x_{cand_ids[t]}|^2) (closest=None: +inf, the pass that forms
    `closest` from the first centre), and part float64 [T, S], the sums of mins[t] over the S fixed row spans.  The distances are direct sums of
    squared differences.  cand_ids: int32 [T] on the device, T <= 16; ids outside [0, N) are clamped."""
    X = _table(X, 'X', 'kmeanspp_dist')
    N, d = X.shape
    cand_ids = _ids(cand_ids, 'cand_ids', 'kmeanspp_dist', X.device)
    if closest is not None:
        if not isinstance(closest, torch.Tensor) or closest.dtype != torch.float32 or closest.shape != (N,) or closest.device != X.device:
            raise ValueError('kmeanspp_dist: closest must be float32 [N] on the device of X')
        closest = closest.contiguous()
    L, T = _lib.lib(), cand_ids.shape[0]
    mins = torch.empty(T, N, dtype=torch.float32, device=X.device)
    part = torch.empty(T, L.arl_kmeanspp_spans(N), dtype=torch.float64, device=X.device)
    check(L.arl_kmeanspp_dist_f32(ops._ptr(X), N, d, ops._ptr(cand_ids), T, None if closest is None else ops._ptr(closest), ops._ptr(mins), ops._ptr(part),
                                  ops._stream()), 'arl_kmeanspp_dist_f32')
    return mins, part


def kmeanspp_pick(mins, part, cand_ids, u=None):
    """The end of a step, from kmeanspp_dist's outputs: (winner int32 [2] = the lowest t with the smallest potential and its row cand_ids[t], cand_pot
    float64 [T] = part folded per candidate, closest float32 [N] = mins[winner], next_ids int32 [len(u)] or None).  next_ids[j] is the first row whose
    inclusive running sum of `closest` reaches u[j] * cand_pot[winner] (numpy.searchsorted on the cumulative sum, clipped to N - 1).  u: float64 on the device."""
    if not isinstance(mins, torch.Tensor) or mins.dtype != torch.float32 or mins.dim() != 2 or not mins.is_cuda or not 1 <= mins.shape[0] <= KMEANSPP_MAX_TRIALS \
            or not 1 <= mins.shape[1] <= (2 ** 31 - 1) // 128:
        raise ValueError('kmeanspp_pick: mins must be float32 [T, N] on the GPU, 1 <= T <= %d' % KMEANSPP_MAX_TRIALS)
    (T, N), L = mins.shape, _lib.lib()
    cand_ids = _ids(cand_ids, 'cand_ids', 'kmeanspp_pick', mins.device)
    if not isinstance(part, torch.Tensor) or part.dtype != torch.float64 or part.shape != (T, L.arl_kmeanspp_spans(N)) or part.device != mins.device \
            or cand_ids.shape[0] != T:
        raise ValueError('kmeanspp_pick: part must be float64 [T, spans(N)] and cand_ids int32 [T] on the device of mins')
    n_next = 0
    if u is not None:
        if not isinstance(u, torch.Tensor) or u.dtype != torch.float64 or u.dim() != 1 or not 1 <= u.shape[0] <= KMEANSPP_MAX_TRIALS or u.device != mins.device:
            raise ValueError('kmeanspp_pick: u must be float64 [T_next], 1 <= T_next <= %d, on the device of mins' % KMEANSPP_MAX_TRIALS)
        u, n_next = u.contiguous(), u.shape[0]
    mins, part = mins.contiguous(), part.contiguous()
    winner = torch.empty(2, dtype=torch.int32, device=mins.device)
    cand_pot = torch.empty(T, dtype=torch.float64, device=mins.device)
    closest = torch.empty(N, dtype=torch.float32, device=mins.device)
    next_ids = torch.empty(n_next, dtype=torch.int32, device=mins.device) if n_next else None
    check(L.arl_kmeanspp_pick_f64(ops._ptr(mins), ops._ptr(part), N, T, ops._ptr(cand_ids), ops._ptr(u) if n_next else None, n_next,
                                  ops._ptr(next_ids) if n_next else None, ops._ptr(winner), ops._ptr(cand_pot), ops._ptr(closest), ops._stream()),
          'arl_kmeanspp_pick_f64')
    return winner, cand_pot, closest, next_ids


def kmeanspp(X, k, draws=None, trace=False):
    """indices int64 [k] on the device of X: the rows greedy k-means++ picks as the start of k clusters of the rows of X [N, d] (float32, on the GPU).
    draws: (first, u) as kmeanspp_draws returns them (u float64 [k - 1, T], 1 <= T <= 16, host or device), else drawn here.  With trace=True also
    cand_ids int32 [k - 1, T] and cand_pot float64 [k - 1, T], every step's candidates and their potentials, and the final closest float32 [N].
    All k - 1 steps are enqueued at once; nothing is read back.  ValueError for N < k, k < 1, an unsupported width, a host or non-float32 table
    (the generator is not advanced then): there is no other route."""
    k = int(k)
    if k < 1:
        raise ValueError('kmeanspp: k = %d, at least one cluster needed' % k)
    if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[0] < k:
        raise ValueError('kmeanspp: n_samples=%d should be >= n_clusters=%d' % (X.shape[0], k))
    X = _table(X, 'X', 'kmeanspp')
    N, d = X.shape
    first, u = kmeanspp_draws(N, k) if draws is None else draws
    first = int(first)
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float64))
    if not isinstance(u, torch.Tensor) or u.dtype != torch.float64 or u.dim() != 2 or u.shape[0] != k - 1 or not 1 <= u.shape[1] <= KMEANSPP_MAX_TRIALS \
            or not 0 <= first < N:
        raise ValueError('kmeanspp: draws must be (first row in [0, N), u float64 [k - 1, T] with 1 <= T <= %d)' % KMEANSPP_MAX_TRIALS)
    u = u.to(X.device).contiguous()
    T, L = u.shape[1], _lib.lib()
    indices = torch.empty(k, dtype=torch.int32, device=X.device)
    closest = torch.empty(N, dtype=torch.float32, device=X.device)
    ws = torch.empty(L.arl_kmeanspp_workspace_bytes(N, T), dtype=torch.uint8, device=X.device)
    cand_ids = cand_pot = None
    if trace:
        cand_ids = torch.empty(k - 1, T, dtype=torch.int32, device=X.device)
        cand_pot = torch.empty(k - 1, T, dtype=torch.float64, device=X.device)
    check(L.arl_kmeanspp_f32(ops._ptr(X), N, d, k, T, first, ops._ptr(u) if k > 1 else None, ops._ptr(indices), ops._ptr(closest),
                             ops._ptr(cand_ids) if trace and k > 1 else None, ops._ptr(cand_pot) if trace and k > 1 else None, ops._ptr(ws), ops._stream()),
          'arl_kmeanspp_f32')
    indices = indices.to(torch.int64)
    return (indices, cand_ids, cand_pot, closest) if trace else indices

"""Full-ranking attack metrics (csrc/arl_targetrank.hip): the rank of each target item for each user over the whole catalogue as tensor-level ops --
the streaming kernel, the composed torch route past its limits, and the dispatcher.  Re-exported by arlib_amd.ops; the limits below are read from
THIS module.

With s = Pu Pi^T [U, I] in fp32 as the route computes it:
    rank[u, t] = #{ j != targets[t], (u, j) not masked : s[u, j] > s[u, targets[t]] or (s[u, j] == s[u, targets[t]] and j < targets[t]) },
the 0-based position of the target in a descending sort of user u's row with ties broken by item id, and -1 where (u, targets[t]) is itself masked.
tscore[u, t] = s[u, targets[t]].  Every number of the reference's AttackMetric (util/metrics.py:125-208) at any k is a function of this matrix."""
import torch

from . import _lib
from ._lib import check
from .allpairs import ALLPAIRS_MAX_ROWS


def _ops():
    from . import ops
    return ops


TARGETRANK_WIDTHS = (16, 32, 64, 128)
TARGETRANK_MAX_TARGETS = 64                    # the limit cw_topk_term has
TARGETRANK_MAX_ROWS = ALLPAIRS_MAX_ROWS        # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
TARGETRANK_CHUNK = 128                         # user rows per panel of the composed route


def target_rank_supported(U, I, d, T, nnz=0):
    """True when the streaming kernel takes the shape; everything else goes through target_rank_composed."""
    U, I, d, T, nnz = int(U), int(I), int(d), int(T), int(nnz)
    return (d in TARGETRANK_WIDTHS and 1 <= T <= TARGETRANK_MAX_TARGETS and 1 <= U <= TARGETRANK_MAX_ROWS and 1 <= I <= TARGETRANK_MAX_ROWS
            and 0 <= nnz < 2 ** 31)


def _rank_args(Pu, Pi, targets, mask, what, on_gpu, check_range):
    """Shapes, dtypes and (check_range) one host read of the index arrays.  Returns (targets int32 [T], mask_rowptr | None, mask_col | None)."""
    if on_gpu:
        o = _ops()
        o._dev(Pu, torch.float32, 'Pu', 2); o._dev(Pi, torch.float32, 'Pi', 2)
    for name, t in (('Pu', Pu), ('Pi', Pi)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('%s: %s must be a torch.Tensor' % (what, name))
        if t.dtype != torch.float32 or t.dim() != 2 or not t.is_contiguous():
            raise TypeError('%s: %s must be a contiguous fp32 matrix' % (what, name))
    (U, d), I = Pu.shape, Pi.shape[0]
    if Pi.shape[1] != d or U == 0 or I == 0 or Pi.device != Pu.device:
        raise ValueError('%s: Pu [U, d] and Pi [I, d] on one device with U, I >= 1' % what)
    if not isinstance(targets, torch.Tensor):
        targets = torch.as_tensor(targets, dtype=torch.int32)
    if targets.dtype != torch.int32 or targets.dim() != 1:
        raise TypeError('%s: targets must be an int32 vector' % what)
    targets = targets.to(Pu.device).contiguous()
    if targets.numel() == 0:
        raise ValueError('%s: at least one target' % what)
    rowptr = col = None
    if mask is not None:
        if len(mask) != 2 or mask[0] is None or mask[1] is None:
            raise ValueError('%s: mask = (rowptr [U + 1], col [nnz]), both halves' % what)
        rowptr, col = mask
        for name, t in (('mask rowptr', rowptr), ('mask col', col)):
            if on_gpu:
                _ops()._dev(t, torch.int32, name, 1)
            if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != Pu.device:
                raise TypeError('%s: %s must be a contiguous int32 vector on the tables\' device' % (what, name))
        if rowptr.numel() != U + 1:
            raise ValueError('%s: mask rowptr [U + 1]' % what)
    if check_range:                                    # the kernels trust the index arrays: one host read before any launch
        tg = targets.long()
        bad = (tg.min() < 0) | (tg.max() >= I) | (torch.unique(tg).numel() != tg.numel())
        if bool(bad):
            raise IndexError('%s: targets must be distinct and lie in [0, I)' % what)
        if rowptr is not None:
            nnz = col.numel()
            bad = (rowptr[0] != 0) | (rowptr[-1] != nnz) | ((rowptr[1:] < rowptr[:-1]).any())
            if bool(bad):
                raise IndexError('%s: mask rowptr must run from 0 to nnz without decreasing' % what)
            if nnz:
                bad = (col.min() < 0) | (col.max() >= I)
                if nnz > 1:                            # each row sorted and distinct (the contract of score_mask_topk)
                    first = torch.zeros(nnz + 1, dtype=torch.bool, device=col.device)
                    first[rowptr[:-1].long()] = True
                    bad = bad | ((col[1:] <= col[:-1]) & ~first[1:nnz]).any()
                if bool(bad):
                    raise IndexError('%s: mask col must lie in [0, I), each row sorted and distinct' % what)
    return targets, rowptr, col


def target_rank_kernel(Pu, Pi, targets, mask=None, check_range=True):
    """The streaming kernel.  Pu [U, d], Pi [I, d] fp32 device tensors; targets [T] int32 (distinct, in [0, I)); mask = (rowptr [U + 1], col [nnz])
    int32 device tensors, the (u, j) pairs to leave out of the count, each row sorted and distinct.  Returns (rank [U, T] int32, tscore [U, T] fp32).
    Shapes outside target_rank_supported raise.  check_range=False skips the host read that validates the index arrays."""
    targets, rowptr, col = _rank_args(Pu, Pi, targets, mask, 'target_rank_kernel', True, check_range)
    (U, d), I, T = Pu.shape, Pi.shape[0], targets.numel()
    nnz = col.numel() if col is not None else 0
    if not target_rank_supported(U, I, d, T, nnz):
        raise ValueError('target_rank_kernel: U = %d, I = %d, d = %d, T = %d outside the kernel\'s limits (d in %s, T <= %d, rows <= %d): use '
                         'target_rank_composed' % (U, I, d, T, TARGETRANK_WIDTHS, TARGETRANK_MAX_TARGETS, TARGETRANK_MAX_ROWS))
    dev = Pu.device
    if col is not None and nnz == 0:                   # an empty tensor has no address: the entry takes one placeholder it never reads
        col = torch.zeros(1, dtype=torch.int32, device=dev)
    L, _ptr = _lib.lib(), _ops()._ptr
    ws = torch.empty(max(L.arl_target_rank_workspace_bytes(U, I, d, T), 16), dtype=torch.uint8, device=dev)
    rank, tscore = torch.empty(U, T, dtype=torch.int32, device=dev), torch.empty(U, T, dtype=torch.float32, device=dev)
    check(L.arl_target_rank_f32(_ptr(Pu), U, _ptr(Pi), I, d, _ptr(targets), T, _ptr(rowptr), _ptr(col), _ptr(rank), _ptr(tscore), _ptr(ws), _ops()._stream()),
          'arl_target_rank_f32')
    return rank, tscore


def target_rank_composed(Pu, Pi, targets, mask=None, chunk=TARGETRANK_CHUNK, check_range=True):
    """The same quantities composed from torch ops in fp32, in panels of `chunk` user rows: Pu[b:e] @ Pi.T, compare and count per target, the mask
    through an index_put_ panel.  The route past the kernel's limits and the yardstick of the tests and tools/rank_bench.py; runs on CPU tensors too.
    Peak memory: a few chunk x I panels."""
    targets, rowptr, col = _rank_args(Pu, Pi, targets, mask, 'target_rank_composed', False, check_range)
    (U, _), I, T = Pu.shape, Pi.shape[0], targets.numel()
    dev = Pu.device
    tg = targets.long()
    tg_host = tg.tolist()
    ids = torch.arange(I, device=dev)
    rank, tscore = torch.empty(U, T, dtype=torch.int32, device=dev), torch.empty(U, T, dtype=torch.float32, device=dev)
    if rowptr is not None:
        nnz = col.numel()
        rows = torch.repeat_interleave(torch.arange(U, device=dev), (rowptr[1:] - rowptr[:-1]).long(), output_size=nnz)
        cols = col.long()
        rp = rowptr.long().cpu()
    for b in range(0, U, chunk):
        e = min(U, b + chunk)
        s = Pu[b:e] @ Pi.t()
        ts = s[:, tg]
        keep = None
        if rowptr is not None:
            lo, hi = int(rp[b]), int(rp[e])
            listed = torch.zeros(e - b, I, dtype=torch.bool, device=dev)
            listed.index_put_((rows[lo:hi] - b, cols[lo:hi]), torch.ones((), dtype=torch.bool, device=dev))
            keep = ~listed
        for t in range(T):
            thr = ts[:, t:t + 1]
            beats = (s > thr) | ((s == thr) & (ids < tg_host[t])[None, :])
            if keep is not None:
                beats &= keep
            r = beats.sum(1).to(torch.int32)
            if keep is not None:
                r = torch.where(listed[:, tg_host[t]], torch.full_like(r, -1), r)
            rank[b:e, t] = r
        tscore[b:e] = ts
    return rank, tscore


def target_rank(Pu, Pi, targets, mask=None, check_range=True):
    """target_rank_kernel where the kernel takes the shape, target_rank_composed otherwise -- past the limits, and for tables that live in host
    memory, where there is no kernel to run (a model evaluated on the CPU)."""
    T = targets.numel() if isinstance(targets, torch.Tensor) else len(targets)
    nnz = mask[1].numel() if mask is not None and len(mask) == 2 and isinstance(mask[1], torch.Tensor) else 0
    if Pu.is_cuda and target_rank_supported(Pu.shape[0], Pi.shape[0], Pu.shape[1], T, nnz):
        return target_rank_kernel(Pu, Pi, targets, mask, check_range)
    return target_rank_composed(Pu, Pi, targets, mask, check_range=check_range)

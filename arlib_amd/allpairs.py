"""GSPAttack's L_per (csrc/arl_allpairs.hip; reference attack/Black/GSPAttack.py:63-75) as tensor-level ops: a binary cross-entropy over every
score of s = Pu Pi^T [R, I] against a sparse target matrix -- the streaming kernel, the composed torch route past its limits, and the dispatcher.
Re-exported by arlib_amd.ops; the limits below are read from THIS module.

With f0(s) = -log(sigmoid(-s) + eps) and f1(s) = -log(sigmoid(s) + eps) (the reference's 1 - sigmoid(s) evaluated as sigmoid(-s)):
    rowloss[r] = sum_i f0(s[r, i]) + sum_{(r, c) listed} a (f1 - f0)(s[r, c]),      loss = sum_r row_weight[r] rowloss[r],
and dPu, dPi are the gradients of upstream * loss."""
import torch

from . import _lib
from ._lib import check


def _ops():
    from . import ops
    return ops


ALLPAIRS_WIDTHS = (16, 32, 64, 128)
ALLPAIRS_MAX_ROWS = (2 ** 31 - 1) // 128       # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
ALLPAIRS_CHUNK = 128                           # rows per panel of the composed route (the reference's batchSize, GSPAttack.py:53)


def bce_allpairs_supported(R, I, d, nnz):
    """True when the streaming kernel takes the shape; everything else goes through bce_allpairs_loss_composed."""
    R, I, d, nnz = int(R), int(I), int(d), int(nnz)
    return d in ALLPAIRS_WIDTHS and 1 <= R <= ALLPAIRS_MAX_ROWS and 1 <= I <= ALLPAIRS_MAX_ROWS and 0 <= nnz < 2 ** 31


def batch_mean_row_weights(R, I, batch=ALLPAIRS_CHUNK, dtype=torch.float32, device=None):
    """The reference's L_per is the mean over ceil(R / batch) batches of each batch's own mean over its rows x I entries (GSPAttack.py:71-75);
    with a ragged last batch that is not the global mean.  It equals sum_r rw[r] sum_i bce[r, i] with rw[r] = 1 / (n_batches * rows_in_batch(r) * I):
    this returns rw [R] (computed in float64).  Rows may be sliced from it."""
    R, I, batch = int(R), int(I), int(batch)
    if R < 1 or I < 1 or batch < 1:
        raise ValueError('batch_mean_row_weights: R, I, batch >= 1')
    n_batches = (R + batch - 1) // batch
    rows = torch.full((R,), float(batch), dtype=torch.float64)
    rows[(n_batches - 1) * batch:] = float(R - (n_batches - 1) * batch)
    return (1.0 / (float(n_batches) * float(I) * rows)).to(dtype=dtype, device=device)


def transpose_positives(rowptr, col, R, I):
    """The by-item form of a by-row CSR, on the device: (post_rowptr [I + 1], post_col [nnz] row ids, post_perm [nnz] positions in the by-row arrays),
    entries of an item in ascending by-row position (a stable sort)."""
    nnz = col.numel()
    rows = torch.repeat_interleave(torch.arange(R, dtype=torch.int32, device=col.device), (rowptr[1:] - rowptr[:-1]).long(), output_size=nnz)
    _, order = torch.sort(col, stable=True)
    post_rowptr = torch.zeros(I + 1, dtype=torch.int32, device=col.device)
    post_rowptr[1:] = torch.cumsum(torch.bincount(col.long(), minlength=I), 0).to(torch.int32)
    return post_rowptr, rows[order].contiguous(), order.to(torch.int32)


def _allpairs_args(Pu, Pi, pos, row_weight, what, check_range=True):
    o = _ops()
    o._dev(Pu, torch.float32, 'Pu', 2); o._dev(Pi, torch.float32, 'Pi', 2); o._dev(row_weight, torch.float32, 'row_weight', 1)
    (R, d), I = Pu.shape, Pi.shape[0]
    if Pi.shape[1] != d or R == 0 or I == 0 or row_weight.numel() != R:
        raise ValueError('%s: Pu [R, d], Pi [I, d] and row_weight [R] with R, I >= 1' % what)
    if len(pos) not in (2, 3):
        raise ValueError('%s: pos = (rowptr, col[, val])' % what)
    rowptr, col = o._dev(pos[0], torch.int32, 'pos rowptr', 1), o._dev(pos[1], torch.int32, 'pos col', 1)
    val = o._dev(pos[2], torch.float32, 'pos val', 1) if len(pos) == 3 and pos[2] is not None else None
    nnz = col.numel()
    if rowptr.numel() != R + 1 or (val is not None and val.numel() != nnz):
        raise ValueError('%s: rowptr [R + 1], col [nnz], val [nnz]' % what)
    if check_range:                                    # the kernels trust the index arrays: one host read before any launch
        bad = (rowptr[0] != 0) | (rowptr[-1] != nnz) | ((rowptr[1:] < rowptr[:-1]).any())
        if nnz:
            bad = bad | (col.min() < 0) | (col.max() >= I)
        if bool(bad):
            raise IndexError('%s: rowptr must run from 0 to nnz without decreasing and col must lie in [0, I)' % what)
    return rowptr, col, val


def _check_transposed(pos_t, R, I, nnz, has_val, what, check_range):
    o = _ops()
    if len(pos_t) not in (2, 3):
        raise ValueError('%s: pos_t = (rowptr, col[, perm])' % what)
    trowptr, tcol = o._dev(pos_t[0], torch.int32, 'pos_t rowptr', 1), o._dev(pos_t[1], torch.int32, 'pos_t col', 1)
    tperm = o._dev(pos_t[2], torch.int32, 'pos_t perm', 1) if len(pos_t) == 3 and pos_t[2] is not None else None
    if trowptr.numel() != I + 1 or tcol.numel() != nnz or (tperm is not None and tperm.numel() != nnz) or (has_val and tperm is None):
        raise ValueError('%s: pos_t rowptr [I + 1], col [nnz], perm [nnz] (perm is needed with weights)' % what)
    if check_range:
        bad = (trowptr[0] != 0) | (trowptr[-1] != nnz) | ((trowptr[1:] < trowptr[:-1]).any())
        if nnz:
            bad = bad | (tcol.min() < 0) | (tcol.max() >= R)
            if tperm is not None:
                bad = bad | (tperm.min() < 0) | (tperm.max() >= nnz)
        if bool(bad):
            raise IndexError('%s: pos_t rowptr must run from 0 to nnz without decreasing, its col in [0, R), its perm in [0, nnz)' % what)
    return trowptr, tcol, tperm


def bce_allpairs_loss(Pu, Pi, pos, row_weight, eps=1e-7, want_grad=False, upstream=1.0, pos_t=None, check_range=True):
    """The streaming kernel.  Pu [R, d], Pi [I, d] fp32; pos = (rowptr [R + 1], col [nnz][, val [nnz]]) int32 device tensors, the positives by row
    with their weights (none: all 1; a repeated entry counts as often as it is listed); pos_t = (rowptr [I + 1], col [nnz] row ids[, perm [nnz]]) the
    same set by item, built on the device when not given and gradients are wanted.  Returns (loss [1], rowloss [R]), with want_grad
    (loss, rowloss, dPu, dPi) where the gradients are those of upstream * loss.  Shapes outside bce_allpairs_supported raise.
    check_range=False skips the host read that validates the index arrays (a caller that built them from a validated matrix)."""
    rowptr, col, val = _allpairs_args(Pu, Pi, pos, row_weight, 'bce_allpairs_loss', check_range)
    (R, d), I, nnz = Pu.shape, Pi.shape[0], col.numel()
    if not bce_allpairs_supported(R, I, d, nnz):
        raise ValueError('bce_allpairs_loss: R = %d, I = %d, d = %d outside the kernel\'s limits (d in %s, rows <= %d): use bce_allpairs_loss_composed'
                         % (R, I, d, ALLPAIRS_WIDTHS, ALLPAIRS_MAX_ROWS))
    dev = Pu.device
    trowptr = tcol = tperm = None
    if want_grad:
        if pos_t is None:
            pos_t = transpose_positives(rowptr, col, R, I)
            trowptr, tcol, tperm = pos_t
        else:
            trowptr, tcol, tperm = _check_transposed(pos_t, R, I, nnz, val is not None, 'bce_allpairs_loss', check_range)
    if nnz == 0:                                       # an empty tensor has no address: the entry takes one placeholder it never reads
        col = torch.zeros(1, dtype=torch.int32, device=dev)
        tcol = col if want_grad else None
    L, _ptr = _lib.lib(), _ops()._ptr
    ws = torch.empty(max(L.arl_bce_allpairs_workspace_bytes(R, I, d, 1 if want_grad else 0), 16), dtype=torch.uint8, device=dev)
    rowloss, loss = torch.empty(R, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    dPu, dPi = (torch.empty_like(Pu), torch.empty_like(Pi)) if want_grad else (None, None)
    check(L.arl_bce_allpairs_f32(_ptr(Pu), R, _ptr(Pi), I, d, _ptr(rowptr), _ptr(col), _ptr(val), _ptr(trowptr), _ptr(tcol), _ptr(tperm if val is not None else None),
                                 _ptr(row_weight), float(eps), float(upstream), _ptr(rowloss), _ptr(loss), _ptr(dPu), _ptr(dPi), _ptr(ws), _ops()._stream()),
          'arl_bce_allpairs_f32')
    return (loss, rowloss, dPu, dPi) if want_grad else (loss, rowloss)


def bce_allpairs_loss_composed(Pu, Pi, pos, row_weight, eps=1e-7, want_grad=False, upstream=1.0, pos_t=None, chunk=ALLPAIRS_CHUNK, check_range=True):
    """The same quantities composed from torch ops in fp32, in panels of `chunk` rows like the reference's batchSize loop (GSPAttack.py:64-75): the
    route past the kernel's limits and the yardstick of the tests and tools/gsp_bench.py.  Peak memory: a few chunk x I panels.  pos_t is not needed."""
    rowptr, col, val = _allpairs_args(Pu, Pi, pos, row_weight, 'bce_allpairs_loss_composed', check_range)
    (R, d), I, nnz = Pu.shape, Pi.shape[0], col.numel()
    dev = Pu.device
    rows = torch.repeat_interleave(torch.arange(R, device=dev), (rowptr[1:] - rowptr[:-1]).long(), output_size=nnz)
    cols = col.long()
    vals = val if val is not None else torch.ones(nnz, dtype=torch.float32, device=dev)
    rp = rowptr.long().cpu()
    rowloss = torch.empty(R, dtype=torch.float32, device=dev)
    dPu, dPi = (torch.empty_like(Pu), torch.zeros_like(Pi)) if want_grad else (None, None)
    for b in range(0, R, chunk):
        e = min(R, b + chunk)
        lo, hi = int(rp[b]), int(rp[e])
        A = torch.zeros(e - b, I, dtype=torch.float32, device=dev)
        A.index_put_((rows[lo:hi] - b, cols[lo:hi]), vals[lo:hi], accumulate=True)
        s = Pu[b:e] @ Pi.t()
        p, q = torch.sigmoid(s), torch.sigmoid(-s)
        f1, f0 = -torch.log(p + eps), -torch.log(q + eps)
        rowloss[b:e] = (f0 + A * (f1 - f0)).sum(1)
        if want_grad:
            pq = p * q
            w0 = pq / (q + eps)
            g = (w0 + A * (-pq / (p + eps) - w0)) * (float(upstream) * row_weight[b:e])[:, None]
            dPu[b:e] = g @ Pi
            dPi += g.t() @ Pu[b:e]
    loss = (row_weight * rowloss).sum().view(1)
    return (loss, rowloss, dPu, dPi) if want_grad else (loss, rowloss)


def bce_allpairs(Pu, Pi, pos, row_weight, eps=1e-7, want_grad=False, upstream=1.0, pos_t=None, check_range=True):
    """bce_allpairs_loss where the kernel takes the shape, bce_allpairs_loss_composed otherwise."""
    if bce_allpairs_supported(Pu.shape[0], Pi.shape[0], Pu.shape[1], pos[1].numel()):
        return bce_allpairs_loss(Pu, Pi, pos, row_weight, eps, want_grad, upstream, pos_t, check_range)
    return bce_allpairs_loss_composed(Pu, Pi, pos, row_weight, eps, want_grad, upstream, check_range=check_range)

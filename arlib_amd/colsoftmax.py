"""LegUP's ranking loss (csrc/arl_colsoftmax.hip; reference attack/Gray/LegUP.py:160-171) as tensor-level ops: the streaming kernel, the composed
torch route past its limits, and the dispatcher.  Re-exported by arlib_amd.ops; the limits below are read from THIS module."""
import numpy as np
import torch

from . import _lib
from ._lib import check


def _ops():
    from . import ops
    return ops


COLSOFTMAX_WIDTHS = (16, 32, 64, 128)
COLSOFTMAX_MAX_ROWS = (2 ** 31 - 1) // 128     # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
COLSOFTMAX_MAX_TARGETS = 1024
COLSOFTMAX_CHUNK = 128                         # user rows per panel of the composed route (the reference's batchSize, LegUP.py:52)


def colsoftmax_target_supported(U, I, d, T):
    """True when the streaming kernel takes the shape; everything else goes through colsoftmax_target_loss_composed."""
    U, I, d, T = int(U), int(I), int(d), int(T)
    return d in COLSOFTMAX_WIDTHS and 1 <= U <= COLSOFTMAX_MAX_ROWS and 1 <= I <= COLSOFTMAX_MAX_ROWS and 1 <= T <= COLSOFTMAX_MAX_TARGETS


def _colsoftmax_args(Pu, Pi, targets, what):
    o = _ops()
    o._dev(Pu, torch.float32, 'Pu', 2); o._dev(Pi, torch.float32, 'Pi', 2)
    if Pu.shape[1] != Pi.shape[1] or Pu.shape[0] == 0 or Pi.shape[0] == 0:
        raise ValueError('%s: Pu [U, d] and Pi [I, d] with U, I >= 1' % what)
    t = np.asarray(targets.cpu() if isinstance(targets, torch.Tensor) else targets, dtype=np.int64).reshape(-1)
    if t.size == 0 or int(t.min()) < 0 or int(t.max()) >= Pi.shape[0]:
        raise IndexError('%s: 1 <= T target column ids in [0, I) needed' % what)
    return t


def colsoftmax_target_loss(Pu, Pi, targets, want_grad=False):
    """LegUP's L_RS (attack/Gray/LegUP.py:160-171) for s = Pu Pi^T [U, I], which is never stored: lse [I] = log sum_u exp(s[u, i]) (a softmax
    over the users of every item column) and loss [1] = -(I sum_u sum_t s[u, c_t] - U T sum_i lse[i]) = -sum_{u, t, i} (s[u, c_t] - lse[i]),
    the closed form of the reference's [U, T, I] broadcast.  targets: the T column ids c_t (host list / array or a tensor; a repeated id counts
    as often as it is listed).  Returns (loss, lse), with want_grad (loss, lse, dPu, dPi).  Shapes outside colsoftmax_target_supported raise."""
    t = _colsoftmax_args(Pu, Pi, targets, 'colsoftmax_target_loss')
    (U, d), I, T = Pu.shape, Pi.shape[0], t.size
    if not colsoftmax_target_supported(U, I, d, T):
        raise ValueError('colsoftmax_target_loss: U = %d, I = %d, d = %d, T = %d outside the kernel\'s limits (d in %s, rows <= %d, T <= %d): '
                         'use colsoftmax_target_loss_composed' % (U, I, d, T, COLSOFTMAX_WIDTHS, COLSOFTMAX_MAX_ROWS, COLSOFTMAX_MAX_TARGETS))
    L, _ptr = _lib.lib(), _ops()._ptr
    tg = torch.from_numpy(t.astype(np.int32)).to(Pu.device)
    ws = torch.empty(max(L.arl_colsoftmax_target_workspace_bytes(U, I, d, 1 if want_grad else 0), 16), dtype=torch.uint8, device=Pu.device)
    lse, loss = torch.empty(I, dtype=torch.float32, device=Pu.device), torch.empty(1, dtype=torch.float32, device=Pu.device)
    dPu, dPi = (torch.empty_like(Pu), torch.empty_like(Pi)) if want_grad else (None, None)
    check(L.arl_colsoftmax_target_loss_f32(_ptr(Pu), U, _ptr(Pi), I, d, _ptr(tg), T, _ptr(lse), _ptr(loss), _ptr(dPu), _ptr(dPi), _ptr(ws), _ops()._stream()),
          'arl_colsoftmax_target_loss_f32')
    return (loss, lse, dPu, dPi) if want_grad else (loss, lse)


def colsoftmax_target_loss_composed(Pu, Pi, targets, want_grad=False, chunk=COLSOFTMAX_CHUNK):
    """The same quantities composed from torch ops in fp32, in panels of `chunk` user rows like the reference's batchSize loop (LegUP.py:163-164):
    the route past the kernel's limits and the yardstick of the tests and tools/legup_bench.py.  Peak memory: one chunk x I panel."""
    t = _colsoftmax_args(Pu, Pi, targets, 'colsoftmax_target_loss_composed')
    (U, d), I, T = Pu.shape, Pi.shape[0], t.size
    tg = torch.from_numpy(t).to(Pu.device)
    lse = torch.full((I,), float('-inf'), dtype=torch.float32, device=Pu.device)
    tsum = torch.zeros((), dtype=torch.float32, device=Pu.device)
    for b in range(0, U, chunk):
        s = Pu[b:b + chunk] @ Pi.t()
        lse = torch.logaddexp(lse, torch.logsumexp(s, 0))
        tsum = tsum + s[:, tg].sum()
    loss = (-(float(I) * tsum - float(U) * float(T) * lse.sum())).view(1)
    if not want_grad:
        return loss, lse
    dPu, dPi = torch.empty_like(Pu), torch.zeros_like(Pi)
    pull = float(I) * Pi[tg].sum(0)
    for b in range(0, U, chunk):
        P = torch.exp(Pu[b:b + chunk] @ Pi.t() - lse)
        dPu[b:b + chunk] = float(U) * float(T) * (P @ Pi) - pull
        dPi += float(U) * float(T) * (P.t() @ Pu[b:b + chunk])
    dPi.index_add_(0, tg, (-float(I) * Pu.sum(0)).expand(T, d).contiguous())
    return loss, lse, dPu, dPi


def colsoftmax_target(Pu, Pi, targets, want_grad=False):
    """colsoftmax_target_loss where the kernel takes the shape, colsoftmax_target_loss_composed otherwise."""
    if colsoftmax_target_supported(Pu.shape[0], Pi.shape[0], Pu.shape[1], len(targets)):
        return colsoftmax_target_loss(Pu, Pi, targets, want_grad)
    return colsoftmax_target_loss_composed(Pu, Pi, targets, want_grad)

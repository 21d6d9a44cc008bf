"""The multinomial likelihood of the autoencoder recommenders (csrc/arl_multinomial.hip; Mult-DAE / Mult-VAE, Liang et al., WWW'18; the reference has no
such model) as tensor-level ops: a softmax over every item of z = q E^T [B, I] for each batch row, read at the row's positives -- the streaming kernel,
the composed torch route past its limits, the dispatcher and the autograd function.  Re-exported by arlib_amd.ops; the limits below are read from
THIS module.

With lse_b = log sum_i exp z_bi, n_b = sum_{i in pos(b)} w_bi and p = softmax_i(z):
    nll[b] = n_b lse_b - sum_{i in pos(b)} w_bi z_bi
    dq[b]  = g_b ( n_b sum_i p_bi E_i - sum_{i in pos(b)} w_bi E_i )
    dE[i]  = sum_b g_b ( n_b p_bi - w_bi [i in pos(b)] ) q_b
The positives travel as CSR: positives = (rowptr [B + 1], col [nnz] int32, sorted and distinct within a row[, val [nnz] weights w]); without val every
w is 1.  A row without positives gives nll = 0 and contributes nothing to either gradient."""
import torch

from . import _lib
from ._lib import check
from .allpairs import transpose_positives


def _ops():
    from . import ops
    return ops


MULTINOMIAL_WIDTHS = (16, 32, 64, 128)
MULTINOMIAL_MAX_ROWS = (2 ** 31 - 1) // 128    # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
MULTINOMIAL_CHUNK_ELEMS = 2 ** 24              # the composed route keeps its row panels under this many elements
# 'auto' takes the kernel from this many B * I scores on: the smallest shape at which tools/multvae_bench.py measured it ahead of the composed route
# (500 x 100 000: 3.5 x; 2 048 x 100 000: 5.6 x).  At ml-1M's 500 x 3 706 both routes are launch-bound and the kernel's call lost (0.85 against 0.34 ms),
# so 'auto' stays composed there; nothing between the two sizes was measured (profiles/multvae_bench.json).
MULTINOMIAL_AUTO_MIN_ELEMS = 50_000_000


def multinomial_softmax_supported(B, I, d, nnz=0):
    """True when the streaming kernel takes the shape; everything else goes through multinomial_softmax_composed."""
    B, I, d, nnz = int(B), int(I), int(d), int(nnz)
    return d in MULTINOMIAL_WIDTHS and 1 <= B <= MULTINOMIAL_MAX_ROWS and 1 <= I <= MULTINOMIAL_MAX_ROWS and 0 <= nnz < 2 ** 31


def auto_prefers_kernel(B, I, d):
    """route='auto' picks the kernel only at shapes where it was measured not to lose to the composed route (B * I at least
    MULTINOMIAL_AUTO_MIN_ELEMS; None would mean nothing measured, 'auto' stays composed)."""
    return MULTINOMIAL_AUTO_MIN_ELEMS is not None and int(B) * int(I) >= MULTINOMIAL_AUTO_MIN_ELEMS


def _shapes(q, E, what):
    if q.dim() != 2 or E.dim() != 2 or q.shape[1] != E.shape[1] or q.shape[0] == 0 or E.shape[0] == 0:
        raise ValueError('%s: q [B, d] and E [I, d] with B, I >= 1' % what)
    return q.shape[0], E.shape[0], q.shape[1]


def _positives(positives, B, what):
    if len(positives) not in (2, 3):
        raise ValueError('%s: positives = (rowptr, col[, val])' % what)
    rowptr, col = positives[0], positives[1]
    val = positives[2] if len(positives) == 3 else None
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.dim() != 1 or col.dim() != 1 or rowptr.numel() != B + 1 or (
            val is not None and (val.dim() != 1 or val.numel() != col.numel())):
        raise ValueError('%s: rowptr [B + 1] and col [nnz] int32, val [nnz]' % what)
    return rowptr, col, val


def _check_range(rowptr, col, I, what):
    nnz = col.numel()                                  # the kernel trusts the index arrays: one host read before any launch
    bad = (rowptr[0] != 0) | (rowptr[-1] != nnz) | ((rowptr[1:] < rowptr[:-1]).any())
    if nnz:
        bad = bad | (col.min() < 0) | (col.max() >= I)
    if bool(bad):
        raise IndexError('%s: rowptr must run from 0 to nnz without decreasing and col must lie in [0, I)' % what)


def _kernel_args(q, E, positives, what):
    o = _ops()
    o._dev(q, torch.float32, 'q', 2); o._dev(E, torch.float32, 'E', 2)
    B, I, d = _shapes(q, E, what)
    rowptr, col, val = _positives(positives, B, what)
    if not multinomial_softmax_supported(B, I, d, col.numel()):
        raise ValueError('%s: B = %d, I = %d, d = %d outside the kernel\'s limits (d in %s, rows <= %d, nnz < 2^31): use the composed route'
                         % (what, B, I, d, MULTINOMIAL_WIDTHS, MULTINOMIAL_MAX_ROWS))
    o._dev(rowptr, torch.int32, 'positives rowptr', 1); o._dev(col, torch.int32, 'positives col', 1)
    if val is not None:
        o._dev(val, torch.float32, 'positives val', 1)
    return B, I, d, rowptr, col, val


def multinomial_softmax_kernel(q, E, positives, g=None, want_grad=False, pos_t=None, check_range=True):
    """The streaming kernel.  q [B, d], E [I, d] fp32 device tensors.  Returns (nll [B], lse [B]), with want_grad (nll, lse, dq, dE), the gradients of
    sum_b g[b] nll[b] (g [B] fp32).  pos_t = allpairs.transpose_positives(rowptr, col, B, I), built here when not given and gradients are wanted.
    Shapes outside multinomial_softmax_supported raise.  check_range=False skips the host read that validates the index arrays."""
    B, I, d, rowptr, col, val = _kernel_args(q, E, positives, 'multinomial_softmax_kernel')
    o = _ops()
    nnz = col.numel()
    if check_range:
        _check_range(rowptr, col, I, 'multinomial_softmax_kernel')
    trowptr = tcol = tperm = None
    if want_grad:
        if g is None:
            raise ValueError('multinomial_softmax_kernel: gradients need the upstream g')
        o._dev(g, torch.float32, 'g', 1)
        if g.numel() != B:
            raise ValueError('multinomial_softmax_kernel: g [B]')
        trowptr, tcol, tperm = transpose_positives(rowptr, col, B, I) if pos_t is None else pos_t
        if trowptr.numel() != I + 1 or tcol.numel() != nnz or tperm.numel() != nnz or any(t.dtype != torch.int32 for t in (trowptr, tcol, tperm)):
            raise ValueError('multinomial_softmax_kernel: pos_t = (rowptr [I + 1], col [nnz], perm [nnz]) int32')
    else:
        g = None
    dev = q.device
    if nnz == 0:                                       # an empty tensor has no address: the entry takes one placeholder it never reads
        col = torch.zeros(1, dtype=torch.int32, device=dev)
        val = None
        tcol = tperm = col if want_grad else None
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_multinomial_softmax_workspace_bytes(B, I, d, 1 if want_grad else 0), 16), dtype=torch.uint8, device=dev)
    nll, lse = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    dq, dE = (torch.empty_like(q), torch.empty_like(E)) if want_grad else (None, None)
    check(L.arl_multinomial_softmax_f32(_ptr(q), B, _ptr(E), I, d, _ptr(rowptr), _ptr(col), _ptr(val), nnz, _ptr(trowptr), _ptr(tcol), _ptr(tperm), _ptr(g),
                                        _ptr(nll), _ptr(lse), _ptr(dq), _ptr(dE), _ptr(ws), o._stream()), 'arl_multinomial_softmax_f32')
    return (nll, lse, dq, dE) if want_grad else (nll, lse)


def multinomial_softmax_composed(q, E, positives, g=None, want_grad=False, chunk=None):
    """The same quantities composed from torch ops in the tensors' dtype, in row panels of `chunk` rows (default: panels under 2^24 elements): the only
    route on the CPU, the route past the kernel's limits, and the yardstick of the tests and tools/multvae_bench.py.  Peak memory: a few chunk x I
    panels."""
    B, I, d = _shapes(q, E, 'multinomial_softmax_composed')
    rowptr, col, val = _positives(positives, B, 'multinomial_softmax_composed')
    if want_grad and g is None:
        raise ValueError('multinomial_softmax_composed: gradients need the upstream g')
    rows = max(1, MULTINOMIAL_CHUNK_ELEMS // I) if chunk is None else max(1, int(chunk))
    dev, nnz = q.device, col.numel()
    deg = (rowptr[1:] - rowptr[:-1]).long()
    prow = torch.repeat_interleave(torch.arange(B, device=dev), deg, output_size=nnz)
    pcol = col.long()
    w = val.to(q.dtype) if val is not None else torch.ones(nnz, dtype=q.dtype, device=dev)
    rp = rowptr.long().cpu()
    nll, lse = torch.empty(B, dtype=q.dtype, device=dev), torch.empty(B, dtype=q.dtype, device=dev)
    dq, dE = (torch.empty_like(q), torch.zeros_like(E)) if want_grad else (None, None)
    for b in range(0, B, rows):
        e = min(B, b + rows)
        lo, hi = int(rp[b]), int(rp[e])
        z = q[b:e] @ E.t()
        l = torch.logsumexp(z, dim=1)
        r, c, ww = prow[lo:hi] - b, pcol[lo:hi], w[lo:hi]
        # the row sums over the positives through a dense panel of the weights: index_add_ on the GPU adds with atomics, in an order that changes
        # from run to run; a row's entries are distinct, so the scatter has one writer per element and the sums below have a fixed order
        A = torch.zeros_like(z)
        A[r, c] = ww
        n, swz = A.sum(1), (A * z).sum(1)
        has = deg[b:e] > 0
        lse[b:e] = l
        nll[b:e] = torch.where(has, n * l - swz, torch.zeros_like(l))
        if want_grad:
            a = torch.where(has, g[b:e].to(q.dtype) * n, torch.zeros_like(n))
            dz = torch.exp(z - l[:, None]) * a[:, None] - g[b:e].to(q.dtype)[:, None] * A
            dq[b:e] = dz @ E
            dE += dz.t() @ q[b:e]
    return (nll, lse, dq, dE) if want_grad else (nll, lse)


def multinomial_softmax(q, E, positives, g=None, want_grad=False):
    """multinomial_softmax_kernel where the kernel takes the shape, multinomial_softmax_composed otherwise."""
    if q.dim() == 2 and E.dim() == 2 and q.is_cuda and q.dtype == torch.float32 and multinomial_softmax_supported(q.shape[0], E.shape[0], q.shape[1], positives[1].numel()):
        return multinomial_softmax_kernel(q, E, positives, g, want_grad)
    return multinomial_softmax_composed(q, E, positives, g, want_grad)


class _MultinomialNll(torch.autograd.Function):
    """nll [B] of the rows; the backward runs the gradient passes with the upstream and feeds dq and dE into the graph.  Saved: q, E and the CSR
    positives -- O(B + I) rows and nnz entries, no B x I tensor."""

    @staticmethod
    def forward(ctx, q, E, rowptr, col, val, fused, check_range):
        q, E = q.contiguous(), E.contiguous()
        ctx.save_for_backward(q, E, rowptr, col, val)
        ctx.fused = fused
        pos = (rowptr, col) if val is None else (rowptr, col, val)
        return (multinomial_softmax_kernel(q, E, pos, check_range=check_range) if fused else multinomial_softmax_composed(q, E, pos))[0]

    @staticmethod
    def backward(ctx, g):
        q, E, rowptr, col, val = ctx.saved_tensors
        pos = (rowptr, col) if val is None else (rowptr, col, val)
        g = g.contiguous()
        if ctx.fused:
            _, _, dq, dE = multinomial_softmax_kernel(q, E, pos, g, want_grad=True, check_range=False)
        else:
            _, _, dq, dE = multinomial_softmax_composed(q, E, pos, g, want_grad=True)
        return dq, dE, None, None, None, None, None


def multinomial_nll(q, E, positives, route='auto', check_range=True):
    """nll [B] differentiable in q and E.  route 'fused': the kernel (shapes outside its limits raise); 'composed': torch, CPU or GPU; 'auto': the
    kernel on a GPU at the shapes where it was measured not to lose to the composed route (auto_prefers_kernel).  check_range=False skips the kernel
    route's host read of the index arrays (a caller that built them from a validated matrix)."""
    if route not in ('auto', 'fused', 'composed'):
        raise ValueError("multinomial_nll: route is 'auto', 'fused' or 'composed', not %r" % (route,))
    B, I, d = _shapes(q, E, 'multinomial_nll')
    rowptr, col, val = _positives(positives, B, 'multinomial_nll')
    if route == 'auto':
        route = 'fused' if (q.is_cuda and q.dtype == torch.float32 and multinomial_softmax_supported(B, I, d, col.numel()) and auto_prefers_kernel(B, I, d)) else 'composed'
    if route == 'fused':
        _kernel_args(q.detach().contiguous(), E.detach().contiguous(), positives, 'multinomial_nll')
    return _MultinomialNll.apply(q, E, rowptr, col, val, route == 'fused', bool(check_range))

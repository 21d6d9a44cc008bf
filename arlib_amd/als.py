"""Alternating least squares for implicit feedback (csrc/arl_als.hip; WRMF as published: Hu, Koren, Volinsky, ICDM'08) as tensor-level ops: the Gram
matrix of a table, the exact row update given the other table -- the fused kernel, the composed torch route, the dispatcher -- and the objective.
Re-exported by arlib_amd.ops; the limits below are read from THIS module.

With p_ui = 1 on the stored entries, confidence c_ui = 1 + alpha w_ui (w = 1 or the stored value) and every unobserved pair weighted 1:
    L   = sum_u sum_i c_ui (p_ui - x_u . y_i)^2 + reg (|X|^2 + |Y|^2)                          over ALL (u, i)
    G   = Y^T Y
    A_r = G + alpha sum_{i in P_r} w_ri y_i y_i^T + reg I,   b_r = sum_{i in P_r} (1 + alpha w_ri) y_i,   x_r = A_r^-1 b_r
    L   = sum_u [ x_u^T G x_u + sum_{i in P_u} ((1 + alpha w)(1 - s)^2 - s^2) ] + reg (|X|^2 + |Y|^2),   s = x_u . y_i
The rows travel as CSR: csr = (rowptr [n_rows + 1], col [nnz] int32 in [0, n)[, val [nnz] weights w]); without val every w is 1.  A row without
entries solves to exactly 0.  A row solve is also a FOLD-IN: the rows need not belong to any model."""
import torch

from . import _lib
from ._lib import check


def _ops():
    from . import ops
    return ops


ALS_WIDTHS = (16, 32, 64, 128)
ALS_MAX_ROWS = (2 ** 31 - 1) // 128            # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
ALS_CHUNK_ELEMS = 2 ** 24                      # the composed route keeps its d x d stack under this many elements ...
ALS_GATHER_ELEMS = 2 ** 25                     # ... and its padded gather [rows, longest row, d] under this many
# 'auto' takes the kernel from this many listed rows on.  tools/als_bench.py found no crossover: at ml-1M's shape the kernel's call was ahead of the
# composed route's at every size tried, from ONE row (d 64: 0.12 against 0.42 ms; d 128: 0.31 against 0.52 ms) to all 6 040 (profiles/als_bench.json,
# leg 'crossover'), so on a GPU 'auto' is the kernel wherever the kernel takes the shape.  None would mean nothing measured:
# 'auto' would stay composed.
ALS_AUTO_MIN_ROWS = 1


def als_supported(d, n=1, n_rows=1, nnz=0):
    """True when the kernels take the shape (d the width, n the other table's rows, n_rows the rows solved); everything else goes through the composed
    route."""
    d, n, n_rows, nnz = int(d), int(n), int(n_rows), int(nnz)
    return d in ALS_WIDTHS and 1 <= n <= ALS_MAX_ROWS and 1 <= n_rows <= ALS_MAX_ROWS and 0 <= nnz < 2 ** 31


def auto_prefers_kernel(n_solve, d):
    """route='auto' picks the kernel only where it was measured not to lose to the composed route."""
    return ALS_AUTO_MIN_ROWS is not None and int(n_solve) >= ALS_AUTO_MIN_ROWS


def default_split_len():
    """Rows longer than this many entries are cut into pieces solved as partial (A, b) by separate workgroups."""
    return int(_lib.lib().arl_als_default_split_len())


def _csr(csr, what):
    if len(csr) not in (2, 3):
        raise ValueError('%s: csr = (rowptr, col[, val])' % what)
    rowptr, col = csr[0], csr[1]
    val = csr[2] if len(csr) == 3 else None
    if rowptr.dtype != torch.int32 or col.dtype != torch.int32 or rowptr.dim() != 1 or col.dim() != 1 or rowptr.numel() < 2 or (
            val is not None and (val.dim() != 1 or val.numel() != col.numel())):
        raise ValueError('%s: rowptr [n_rows + 1] and col [nnz] int32, val [nnz]' % what)
    return rowptr, col, val


def _rows(rows, what):
    if rows is not None and (rows.dtype != torch.int32 or rows.dim() != 1 or rows.numel() == 0):
        raise ValueError('%s: rows [n_solve] int32, n_solve >= 1' % what)
    return rows


def _table(Y, what):
    if Y.dim() != 2 or Y.shape[0] == 0:
        raise ValueError('%s: a table [n, d] with n >= 1' % what)
    return Y.shape


def _check_range(rowptr, col, rows, n, what):
    nnz, n_rows = col.numel(), rowptr.numel() - 1             # the kernels trust the index arrays: one host read before any launch
    bad = (rowptr[0] != 0) | (rowptr[-1] != nnz) | ((rowptr[1:] < rowptr[:-1]).any())
    if nnz:
        bad = bad | (col.min() < 0) | (col.max() >= n)
    if rows is not None:
        bad = bad | (rows.min() < 0) | (rows.max() >= n_rows)
    if bool(bad):
        raise IndexError('%s: rowptr must run from 0 to nnz without decreasing, col must lie in [0, n) and rows in [0, n_rows)' % what)


def gram(Y):
    """G = Y^T Y [d, d] in float64: the kernel (fixed spans, fixed order) for an fp32 device table of a supported width, torch in float64 otherwise."""
    n, d = _table(Y, 'gram')
    if not (Y.is_cuda and Y.dtype == torch.float32 and als_supported(d, n)):
        Yd = Y.double()
        return Yd.t() @ Yd
    o = _ops()
    Y = o._dev(Y.contiguous(), torch.float32, 'Y', 2)
    L = _lib.lib()
    ws = torch.empty(max(L.arl_als_gram_workspace_bytes(n, d), 16), dtype=torch.uint8, device=Y.device)
    G = torch.empty(d, d, dtype=torch.float64, device=Y.device)
    check(L.arl_als_gram_f64(o._ptr(Y), n, d, o._ptr(G), o._ptr(ws), o._stream()), 'arl_als_gram_f64')
    return G


def _kernel_args(Y, G, csr, rows, what):
    o = _ops()
    o._dev(Y, torch.float32, 'Y', 2); o._dev(G, torch.float64, 'G', 2)
    n, d = _table(Y, what)
    rowptr, col, val = _csr(csr, what)
    rows = _rows(rows, what)
    n_rows = rowptr.numel() - 1
    if tuple(G.shape) != (d, d):
        raise ValueError('%s: G [d, d]' % what)
    if not als_supported(d, n, n_rows, col.numel()) or (rows is not None and rows.numel() > ALS_MAX_ROWS):
        raise ValueError('%s: n = %d, n_rows = %d, d = %d outside the kernel\'s limits (d in %s, rows <= %d, nnz < 2^31): use the composed route'
                         % (what, n, n_rows, d, ALS_WIDTHS, ALS_MAX_ROWS))
    o._dev(rowptr, torch.int32, 'csr rowptr', 1); o._dev(col, torch.int32, 'csr col', 1)
    if val is not None:
        o._dev(val, torch.float32, 'csr val', 1)
    if rows is not None:
        o._dev(rows, torch.int32, 'rows', 1)
    return n, d, n_rows, rowptr, col, val, rows


def _coefs(alpha, reg, what):
    alpha, reg = float(alpha), float(reg)
    if not alpha >= 0.0 or not reg >= 0.0:
        raise ValueError('%s: alpha >= 0 and reg >= 0' % what)
    return alpha, reg


def als_solve_rows_kernel(Y, G, csr, alpha, reg, rows=None, split_len=None, check_range=True):
    """The fused kernel.  Y [n, d] fp32 and G = gram(Y) [d, d] float64 device tensors.  Returns X [n_solve, d] fp32: row j solves CSR row rows[j]
    (rows int32, repeats and any order allowed), or row j without rows.  split_len: rows longer than it are cut into pieces (default:
    default_split_len()); the result depends on it through the summation order only.  Shapes outside als_supported raise.  check_range=False skips
    the host read that validates the index arrays."""
    what = 'als_solve_rows_kernel'
    n, d, n_rows, rowptr, col, val, rows = _kernel_args(Y, G, csr, rows, what)
    alpha, reg = _coefs(alpha, reg, what)
    if split_len is not None and int(split_len) < 1:
        raise ValueError('%s: split_len >= 1' % what)
    split_len = 0 if split_len is None else int(split_len)          # 0: the entry's default
    o = _ops()
    nnz = col.numel()
    if check_range:
        _check_range(rowptr, col, rows, n, what)
    if rows is None:
        n_solve, listed = n_rows, nnz
    else:
        n_solve = rows.numel()
        listed = int((rowptr[rows.long() + 1].long() - rowptr[rows.long()].long()).sum())      # sizes the pieces' workspace
        if listed >= 2 ** 31:
            raise ValueError('%s: the listed rows hold 2^31 entries or more' % what)
    dev = Y.device
    if nnz == 0:                                       # an empty tensor has no address: the entry takes one placeholder it never reads
        col, val = torch.zeros(1, dtype=torch.int32, device=dev), None
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_als_solve_rows_workspace_bytes(n_solve, listed, d, split_len), 16), dtype=torch.uint8, device=dev)
    X = torch.empty(n_solve, d, dtype=torch.float32, device=dev)
    check(L.arl_als_solve_rows_f32(_ptr(Y), n, d, _ptr(G), _ptr(rowptr), _ptr(col), _ptr(val), n_rows, _ptr(rows), n_solve, listed, alpha, reg, split_len,
                                   _ptr(X), _ptr(ws), o._stream()), 'arl_als_solve_rows_f32')
    return X


def als_solve_rows_composed(Y, G, csr, alpha, reg, rows=None, chunk=None):
    """The same rows composed from torch ops in Y's dtype: a padded gather of the rows' entries, bmm, torch.linalg.cholesky and cholesky_solve, in
    chunks of rows that keep the d x d stack (ALS_CHUNK_ELEMS) and the gather (ALS_GATHER_ELEMS) bounded.  The only route on the CPU, the route
    past the kernel's limits, and the yardstick of the tests and tools/als_bench.py."""
    what = 'als_solve_rows_composed'
    n, d = _table(Y, what)
    rowptr, col, val = _csr(csr, what)
    rows = _rows(rows, what)
    alpha, reg = _coefs(alpha, reg, what)
    if tuple(G.shape) != (d, d):
        raise ValueError('%s: G [d, d]' % what)
    dev, dt, nnz = Y.device, Y.dtype, col.numel()
    rp = rowptr.long()
    sel = torch.arange(rowptr.numel() - 1, device=dev) if rows is None else rows.long()
    n_solve = sel.numel()
    lo_all, deg_all = rp[sel], rp[sel + 1] - rp[sel]
    deg_host = deg_all.cpu()
    X = torch.zeros(n_solve, d, dtype=dt, device=dev)
    if nnz == 0:
        return X
    Gt, eye, col_l = G.to(dt), torch.eye(d, dtype=dt, device=dev), col.long()
    w_all = None if val is None else val.to(dt)
    R0 = max(1, ALS_CHUNK_ELEMS // (d * d)) if chunk is None else max(1, int(chunk))
    b0 = 0
    while b0 < n_solve:
        R = min(R0, n_solve - b0)
        Lmax = int(deg_host[b0:b0 + R].max())
        while R > 1 and R * Lmax * d > ALS_GATHER_ELEMS:
            R //= 2
            Lmax = int(deg_host[b0:b0 + R].max())
        if Lmax > 0:
            lo, deg = lo_all[b0:b0 + R], deg_all[b0:b0 + R]
            pos = torch.arange(Lmax, device=dev)[None, :]
            m = pos < deg[:, None]
            at = torch.where(m, lo[:, None] + pos, torch.zeros_like(pos))
            Yg = Y[col_l[at]]                                                  # [R, Lmax, d]; padded slots carry weight 0
            mf = m.to(dt)
            w = mf if w_all is None else w_all[at] * mf
            c = mf + alpha * w
            S = torch.bmm((Yg * w[..., None]).transpose(1, 2), Yg)
            A = Gt + alpha * S + reg * eye
            b = (c[..., None] * Yg).sum(1)
            x = torch.cholesky_solve(b[..., None], torch.linalg.cholesky(A))[..., 0]
            X[b0:b0 + R] = torch.where((deg > 0)[:, None], x, torch.zeros_like(x))
        b0 += R
    return X


def als_solve_rows(Y, G, csr, alpha, reg, rows=None, route='auto', split_len=None, check_range=True):
    """x_r = A_r^-1 b_r for the listed rows.  route 'fused': the kernel (shapes outside its limits raise); 'composed': torch, CPU or GPU; 'auto': the
    kernel on a GPU at the sizes where it was measured not to lose to the composed route (auto_prefers_kernel)."""
    if route not in ('auto', 'fused', 'composed'):
        raise ValueError("als_solve_rows: route is 'auto', 'fused' or 'composed', not %r" % (route,))
    n, d = _table(Y, 'als_solve_rows')
    rowptr, col, val = _csr(csr, 'als_solve_rows')
    n_solve = rowptr.numel() - 1 if rows is None else rows.numel()
    if route == 'auto':
        route = 'fused' if (Y.is_cuda and Y.dtype == torch.float32 and als_supported(d, n, rowptr.numel() - 1, col.numel())
                            and auto_prefers_kernel(n_solve, d)) else 'composed'
    if route == 'fused':
        return als_solve_rows_kernel(Y.contiguous(), G, csr, alpha, reg, rows, split_len, check_range)
    return als_solve_rows_composed(Y, G, csr, alpha, reg, rows)


def _objective_composed(X, Y, G, rowptr, col, val, alpha, reg):
    Xd, Yd = X.double(), Y.double()
    G = (Yd.t() @ Yd) if G is None else G.double()
    total = ((Xd @ G) * Xd).sum() + reg * ((Xd * Xd).sum() + (Yd * Yd).sum())
    nnz = col.numel()
    if nnz:
        deg = (rowptr[1:] - rowptr[:-1]).long()
        row = torch.repeat_interleave(torch.arange(deg.numel(), device=X.device), deg, output_size=nnz)
        step = max(1, 2 ** 22 // X.shape[1])
        for b in range(0, nnz, step):
            s = (Xd[row[b:b + step]] * Yd[col[b:b + step].long()]).sum(1)
            w = 1.0 if val is None else val[b:b + step].double()
            total = total + ((1.0 + alpha * w) * (1.0 - s) ** 2 - s * s).sum()
    return total


def als_objective(X, Y, csr, alpha, reg, G=None, route='auto', check_range=True):
    """L for the tables X [n_rows, d], Y [n, d] and the CSR of X's rows, a 0-dim float64 tensor, by the Gram identity (no n_rows x n scores).  G =
    gram(Y), computed here when not given.  route 'fused': the kernel; 'composed': torch in float64; 'auto': the kernel for fp32 device tables of a
    supported width."""
    what = 'als_objective'
    if route not in ('auto', 'fused', 'composed'):
        raise ValueError("%s: route is 'auto', 'fused' or 'composed', not %r" % (what, route))
    n, d = _table(Y, what)
    n_rows, dx = _table(X, what)
    rowptr, col, val = _csr(csr, what)
    alpha, reg = _coefs(alpha, reg, what)
    if dx != d or rowptr.numel() != n_rows + 1:
        raise ValueError('%s: X [n_rows, d], Y [n, d] and rowptr [n_rows + 1]' % what)
    if route == 'auto':
        route = 'fused' if (X.is_cuda and X.dtype == torch.float32 and Y.dtype == torch.float32 and als_supported(d, n, n_rows, col.numel())) else 'composed'
    if route == 'composed':
        return _objective_composed(X, Y, G, rowptr, col, val, alpha, reg)
    X, Y = X.contiguous(), Y.contiguous()
    if G is None:
        G = gram(Y)
    _kernel_args(Y, G, csr, None, what)
    o = _ops()
    o._dev(X, torch.float32, 'X', 2)
    if check_range:
        _check_range(rowptr, col, None, n, what)
    dev = X.device
    if col.numel() == 0:
        col, val = torch.zeros(1, dtype=torch.int32, device=dev), None
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_als_objective_workspace_bytes(n_rows, n, d), 16), dtype=torch.uint8, device=dev)
    out = torch.empty(1, dtype=torch.float64, device=dev)
    check(L.arl_als_objective_f64(_ptr(X), n_rows, _ptr(Y), n, d, _ptr(G), _ptr(rowptr), _ptr(col), _ptr(val), alpha, reg, _ptr(out), _ptr(ws), o._stream()),
          'arl_als_objective_f64')
    return out[0]

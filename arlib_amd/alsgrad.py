"""The ALS row solve under a target rule, and its adjoint (csrc/arl_als.hip), as tensor-level ops: the operator that lets an attack differentiate an
adversarial loss through unrolled ALS sweeps exactly (Tang, Wen, Wang, RecSys'20) -- the fused kernels, the composed torch route, the dispatchers,
and als_solve, the differentiable row solve.  Re-exported by arlib_amd.ops; the limits are those of arlib_amd/als.py.

Forward, for row r of the solved table, Y the other table, P_r the row's stored entries with weights w (als.py's CSR; without val every w is 1):
    G   = Y^T Y
    A_r = G + alpha sum_{i in P_r} w_ri y_i y_i^T + reg I,   b_r = sum_{i in P_r} beta(w_ri) y_i,   x_r = A_r^-1 b_r
    target 'stored':  beta(w) = 1 + alpha w      what als_solve_rows computes (p = 1 on every stored entry)
    target 'relaxed': beta(w) = (1 + alpha) w    the same number at w = 1; at w = 0 the entry contributes nothing, exactly as if it were absent: a
                                                 dense row of weights in [0, 1] is a continuous relaxation of a binary profile ('stored' is not: a
                                                 stored entry of weight 0 still pulls x towards y_i)
Adjoint, given g_r = dL/dx_r:  z_r = A_r^-1 g_r,  s = x_r . y_i,  t = z_r . y_i,  C = sum_r z_r x_r^T
    dL/dw_ri = t (beta'(w_ri) - alpha s)                                                       beta' = alpha | 1 + alpha
    dL/dy_i  = sum_{r with i} [ (beta(w_ri) - alpha w_ri s) z_r - alpha w_ri t x_r ]  -  y_i (C + C^T)
The last term is the path through G: als_solve computes G itself, so it belongs to the function.  A row without entries has x = 0 and z = 0 and
contributes nothing whatever its upstream gradient holds."""
import torch

from . import _lib, als
from ._lib import check
from .allpairs import transpose_positives


def _ops():
    from . import ops
    return ops


ALSGRAD_TARGETS = ('stored', 'relaxed')
# 'auto' takes the kernels from this many rows on, by ALS_AUTO_MIN_ROWS' convention (None would mean nothing measured: 'auto' would stay composed).
# tools/alsgrad_bench.py found no crossover: at ml-1M's shape the adjoint kernel's call was ahead of the composed route's at every size tried, from
# ONE row (d 64: 0.11 against 0.99 ms; d 128: 0.26 against 1.49 ms) to all 6 040 (1.02 against 24.8 ms; 3.28 against 48.4 ms) (profiles/alsgrad_bench.json,
# leg 'crossover'), so on a GPU 'auto' is the kernels wherever they take the shape.
ALSGRAD_AUTO_MIN_ROWS = 1


def auto_prefers_kernel(n_rows, d):
    """route='auto' picks the kernels only where they were measured not to lose to the composed route."""
    return ALSGRAD_AUTO_MIN_ROWS is not None and int(n_rows) >= ALSGRAD_AUTO_MIN_ROWS


def default_col_split_len():
    """Columns of the adjoint's column pass longer than this many entries are cut into pieces summed by separate workgroups."""
    return int(_lib.lib().arl_als_default_col_split_len())


def _target(target, what):
    if target not in ALSGRAD_TARGETS:
        raise ValueError("%s: target is 'stored' or 'relaxed', not %r" % (what, target))
    return ALSGRAD_TARGETS.index(target)


def _route(route, what):
    if route not in ('auto', 'fused', 'composed'):
        raise ValueError("%s: route is 'auto', 'fused' or 'composed', not %r" % (what, route))


def _split(split_len, what, name='split_len'):
    if split_len is not None and int(split_len) < 1:
        raise ValueError('%s: %s >= 1' % (what, name))
    return 0 if split_len is None else int(split_len)                  # 0: the entry's default


def _pick(route, Y, n_rows, nnz):
    n, d = Y.shape
    if route != 'auto':
        return route
    return 'fused' if (Y.is_cuda and Y.dtype == torch.float32 and als.als_supported(d, n, n_rows, nnz) and auto_prefers_kernel(n_rows, d)) else 'composed'


def _chunks(ptr, d, dev, chunk=None):
    """The rows of a CSR pointer array in runs that keep a d x d stack (ALS_CHUNK_ELEMS) and a padded gather [rows, longest row, d]
    (ALS_GATHER_ELEMS) bounded, as als_solve_rows_composed cuts them: yields (b0, R, at [R, Lmax] entry positions, m [R, Lmax] the mask of the real
    slots, deg [R]) for every run that holds an entry."""
    ptr = ptr.long()
    n_rows = ptr.numel() - 1
    lo_all, deg_all = ptr[:-1], ptr[1:] - ptr[:-1]
    deg_host = deg_all.cpu()
    R0 = max(1, als.ALS_CHUNK_ELEMS // (d * d)) if chunk is None else max(1, int(chunk))
    b0 = 0
    while b0 < n_rows:
        R = min(R0, n_rows - b0)
        Lmax = int(deg_host[b0:b0 + R].max())
        while R > 1 and R * Lmax * d > als.ALS_GATHER_ELEMS:
            R //= 2
            Lmax = int(deg_host[b0:b0 + R].max())
        if Lmax > 0:
            lo, deg = lo_all[b0:b0 + R], deg_all[b0:b0 + R]
            pos = torch.arange(Lmax, device=dev)[None, :]
            m = pos < deg[:, None]
            yield b0, R, torch.where(m, lo[:, None] + pos, torch.zeros_like(pos)), m, deg
        b0 += R


def _normal_equations(Y, Gt, eye, col_l, w_all, at, m, alpha, reg):
    """(Yg [R, L, d] the gathered rows, w [R, L] the weights with 0 on the padded slots, mf the mask as numbers, A [R, d, d])."""
    Yg = Y[col_l[at]]
    mf = m.to(Y.dtype)
    w = mf if w_all is None else w_all[at] * mf
    A = Gt + alpha * torch.bmm((Yg * w[..., None]).transpose(1, 2), Yg) + reg * eye
    return Yg, w, mf, A


def _beta(w, mf, alpha, target):
    """(beta(w), beta'(w)) on the real slots."""
    if target == 'stored':
        return mf + alpha * w, alpha * mf
    return (1.0 + alpha) * w, (1.0 + alpha) * mf


def _solve_composed(Y, G, rowptr, col, val, alpha, reg, target, chunk=None):
    """als_solve_rows_composed for every row, with the target rule selectable; torch ops throughout, so torch autograd can differentiate it."""
    n, d = Y.shape
    dev, dt = Y.device, Y.dtype
    X = torch.zeros(rowptr.numel() - 1, d, dtype=dt, device=dev)
    if col.numel() == 0:
        return X
    Gt, eye, col_l = G.to(dt), torch.eye(d, dtype=dt, device=dev), col.long()
    w_all = None if val is None else val.to(dt)
    parts, done = [], 0
    for b0, R, at, m, deg in _chunks(rowptr, d, dev, chunk):
        Yg, w, mf, A = _normal_equations(Y, Gt, eye, col_l, w_all, at, m, alpha, reg)
        b = (_beta(w, mf, alpha, target)[0][..., None] * Yg).sum(1)
        x = torch.cholesky_solve(b[..., None], torch.linalg.cholesky(A))[..., 0]
        parts += [X[done:b0], torch.where((deg > 0)[:, None], x, torch.zeros_like(x))]          # runs of empty rows in between stay 0
        done = b0 + R
    return torch.cat(parts + [X[done:]])


def _kernel_shapes(Y, G, csr, split_len, what):
    n, d, n_rows, rowptr, col, val, _ = als._kernel_args(Y, G, csr, None, what)
    return n, d, n_rows, rowptr, col, val, _split(split_len, what)


def als_solve_rows_target(Y, G, csr, alpha, reg, target='stored', route='auto', split_len=None, check_range=True):
    """x_r = A_r^-1 b_r for every row of the CSR under the target rule; no gradient.  route 'fused': the kernel (Y [n, d] fp32 and G = gram(Y) float64
    device tensors; shapes outside als_supported raise) -- under 'stored' exactly what als_solve_rows_kernel returns; 'composed': torch, CPU or GPU;
    'auto': the kernel on a GPU wherever als_solve_rows takes it (als.auto_prefers_kernel)."""
    what = 'als_solve_rows_target'
    _route(route, what)
    tcode = _target(target, what)
    n, d = als._table(Y, what)
    rowptr, col, val = als._csr(csr, what)
    alpha, reg = als._coefs(alpha, reg, what)
    n_rows, nnz = rowptr.numel() - 1, col.numel()
    if route == 'auto':
        route = 'fused' if (Y.is_cuda and Y.dtype == torch.float32 and als.als_supported(d, n, n_rows, nnz) and als.auto_prefers_kernel(n_rows, d)) else 'composed'
    if route == 'composed':
        if tuple(G.shape) != (d, d):
            raise ValueError('%s: G [d, d]' % what)
        with torch.no_grad():
            return _solve_composed(Y, G, rowptr, col, val, alpha, reg, target)
    Y = Y.contiguous()
    n, d, n_rows, rowptr, col, val, split_len = _kernel_shapes(Y, G, csr, split_len, what)
    if check_range:
        als._check_range(rowptr, col, None, n, what)
    o = _ops()
    dev = Y.device
    if nnz == 0:                                       # an empty tensor has no address: the entry takes one placeholder it never reads
        col, val = torch.zeros(1, dtype=torch.int32, device=dev), None
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_als_solve_rows_target_workspace_bytes(n_rows, nnz, d, split_len), 16), dtype=torch.uint8, device=dev)
    X = torch.empty(n_rows, d, dtype=torch.float32, device=dev)
    check(L.arl_als_solve_rows_target_f32(_ptr(Y), n, d, _ptr(G), _ptr(rowptr), _ptr(col), _ptr(val), n_rows, None, n_rows, nnz, alpha, reg, tcode, split_len,
                                          _ptr(X), _ptr(ws), o._stream()), 'arl_als_solve_rows_target_f32')
    return X


def _transposed(transposed, rowptr, col, n_rows, n, what, check_range):
    if transposed is None:
        return transpose_positives(rowptr, col, n_rows, n)
    nnz = col.numel()
    if len(transposed) != 3 or any(t.dtype != torch.int32 or t.dim() != 1 for t in transposed) or transposed[0].numel() != n + 1 or (
            transposed[1].numel() != nnz or transposed[2].numel() != nnz):
        raise ValueError('%s: transposed = (tptr [n + 1], trow [nnz], tperm [nnz]) int32' % what)
    tptr, trow, tperm = transposed
    if check_range and nnz:
        bad = (tptr[0] != 0) | (tptr[-1] != nnz) | ((tptr[1:] < tptr[:-1]).any()) | (trow.min() < 0) | (trow.max() >= n_rows) | (tperm.min() < 0) | (
            tperm.max() >= nnz)
        if bool(bad):
            raise IndexError('%s: tptr must run from 0 to nnz without decreasing, trow must lie in [0, n_rows) and tperm in [0, nnz)' % what)
    return tptr, trow, tperm


def _solved(X, gX, n_rows, d, what):
    if X.dim() != 2 or tuple(X.shape) != (n_rows, d) or tuple(gX.shape) != (n_rows, d):
        raise ValueError('%s: X and gX [n_rows, d], the solved rows and their upstream gradient' % what)


def als_adjoint_kernel(Y, G, csr, X, gX, alpha, reg, target, transposed=None, want_dval=True, split_len=None, col_split_len=None, check_range=True):
    """The fused adjoint.  Y [n, d] fp32, G = gram(Y) float64, X [n_rows, d] = the solved rows and gX [n_rows, d] = dL/dX fp32, all device tensors.
    Returns (dY [n, d] fp32, dval [nnz] fp32 | None without want_dval).  transposed = (tptr, trow, tperm), the by-column order of the CSR
    (allpairs.transpose_positives; built here when None).  split_len cuts long rows as in the forward, col_split_len long columns of the column pass
    (default: default_col_split_len()); the results depend on them through the summation order only.  Shapes outside als_supported raise."""
    what = 'als_adjoint_kernel'
    tcode = _target(target, what)
    n, d, n_rows, rowptr, col, val, split_len = _kernel_shapes(Y, G, csr, split_len, what)
    col_split_len = _split(col_split_len, what, 'col_split_len')
    alpha, reg = als._coefs(alpha, reg, what)
    o = _ops()
    o._dev(X, torch.float32, 'X', 2); o._dev(gX, torch.float32, 'gX', 2)
    _solved(X, gX, n_rows, d, what)
    if check_range:
        als._check_range(rowptr, col, None, n, what)
    dev, nnz = Y.device, col.numel()
    if nnz == 0:                                       # every row is empty: z = 0, C = 0
        return torch.zeros(n, d, dtype=torch.float32, device=dev), (torch.zeros(0, dtype=torch.float32, device=dev) if want_dval else None)
    tptr, trow, tperm = _transposed(transposed, rowptr, col, n_rows, n, what, check_range)
    for t, name in ((tptr, 'tptr'), (trow, 'trow'), (tperm, 'tperm')):
        o._dev(t, torch.int32, name, 1)
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_als_adjoint_workspace_bytes(n, n_rows, nnz, d, split_len, col_split_len), 16), dtype=torch.uint8, device=dev)
    dY = torch.empty(n, d, dtype=torch.float32, device=dev)
    dval = torch.empty(nnz, dtype=torch.float32, device=dev) if want_dval else None
    check(L.arl_als_adjoint_f32(_ptr(Y), n, d, _ptr(G), _ptr(rowptr), _ptr(col), _ptr(val), n_rows, nnz, _ptr(X), _ptr(gX), _ptr(tptr), _ptr(trow), _ptr(tperm),
                                alpha, reg, tcode, split_len, col_split_len, _ptr(dY), _ptr(dval), _ptr(ws), o._stream()), 'arl_als_adjoint_f32')
    return dY, dval


def als_adjoint_composed(Y, G, csr, X, gX, alpha, reg, target, transposed=None, want_dval=True, chunk=None):
    """The same adjoint by the formulas of the module docstring in torch ops, in Y's dtype, CPU or GPU, in chunks of rows (then of columns) that keep
    the d x d stack and the padded gathers bounded as als_solve_rows_composed does.  Every sum has one writer per element and a fixed order.  The only
    route on the CPU, the route past the kernel's limits, and the yardstick of the tests and tools/alsgrad_bench.py."""
    what = 'als_adjoint_composed'
    _target(target, what)
    n, d = als._table(Y, what)
    rowptr, col, val = als._csr(csr, what)
    alpha, reg = als._coefs(alpha, reg, what)
    n_rows, nnz = rowptr.numel() - 1, col.numel()
    if tuple(G.shape) != (d, d):
        raise ValueError('%s: G [d, d]' % what)
    _solved(X, gX, n_rows, d, what)
    dev, dt = Y.device, Y.dtype
    X, gX = X.to(dt), gX.to(dt)
    dY = torch.zeros(n, d, dtype=dt, device=dev)
    dval = torch.zeros(nnz, dtype=dt, device=dev) if want_dval else None
    if nnz == 0:
        return dY, dval
    Gt, eye, col_l = G.to(dt), torch.eye(d, dtype=dt, device=dev), col.long()
    w_all = None if val is None else val.to(dt)
    Z = torch.zeros(n_rows, d, dtype=dt, device=dev)
    ca, cb = torch.zeros(nnz, dtype=dt, device=dev), torch.zeros(nnz, dtype=dt, device=dev)
    for b0, R, at, m, deg in _chunks(rowptr, d, dev, chunk):
        Yg, w, mf, A = _normal_equations(Y, Gt, eye, col_l, w_all, at, m, alpha, reg)
        z = torch.cholesky_solve(gX[b0:b0 + R, :, None], torch.linalg.cholesky(A))[..., 0]
        z = torch.where((deg > 0)[:, None], z, torch.zeros_like(z))
        Z[b0:b0 + R] = z
        s, t = (Yg * X[b0:b0 + R, None, :]).sum(-1), (Yg * z[:, None, :]).sum(-1)
        be, db = _beta(w, mf, alpha, target)
        e = at[m]                                                       # every stored entry once: one writer per element
        ca[e], cb[e] = (be - alpha * w * s)[m], (-alpha * w * t)[m]
        if want_dval:
            dval[e] = (t * (db - alpha * s))[m]
    C = Z.t() @ X
    tptr, trow, tperm = _transposed(transposed, rowptr, col, n_rows, n, what, True)
    trow_l, tperm_l = trow.long(), tperm.long()
    for b0, R, at, m, deg in _chunks(tptr, d, dev, chunk):
        e, r, mf = tperm_l[at], trow_l[at], m.to(dt)
        dY[b0:b0 + R] = ((ca[e] * mf)[..., None] * Z[r] + (cb[e] * mf)[..., None] * X[r]).sum(1)
    dY -= Y @ (C + C.t())
    return dY, dval


def als_adjoint(Y, G, csr, X, gX, alpha, reg, target, transposed=None, want_dval=True, route='auto', split_len=None, col_split_len=None, check_range=True):
    """(dY, dval) of the row solve.  route 'fused': the kernels (shapes outside their limits raise); 'composed': torch, CPU or GPU; 'auto': the kernels
    on a GPU at the sizes where they were measured not to lose to the composed route (auto_prefers_kernel)."""
    what = 'als_adjoint'
    _route(route, what)
    als._table(Y, what)
    rowptr, col, _ = als._csr(csr, what)
    if _pick(route, Y, rowptr.numel() - 1, col.numel()) == 'fused':
        return als_adjoint_kernel(Y.contiguous(), G, csr, X.contiguous(), gX.contiguous(), alpha, reg, target, transposed, want_dval, split_len, col_split_len,
                                  check_range)
    return als_adjoint_composed(Y, G, csr, X, gX, alpha, reg, target, transposed, want_dval)


class _AlsSolve(torch.autograd.Function):
    """X [n_rows, d] of every row; the backward runs the adjoint with the upstream gradient and feeds dY and dval into the graph.  Saved: Y, G, X and the
    CSR -- no n_rows x d x d stack."""

    @staticmethod
    def forward(ctx, Y, val, rowptr, col, tptr, trow, tperm, alpha, reg, target, fused, split_len):
        Y = Y.contiguous()
        G = als.gram(Y)
        csr = (rowptr, col) if val is None else (rowptr, col, val)
        if fused:
            X = als_solve_rows_target(Y, G, csr, alpha, reg, target, 'fused', split_len, check_range=False)
        else:
            X = _solve_composed(Y, G, rowptr, col, val, alpha, reg, target)
        ctx.save_for_backward(Y, G, X, val, rowptr, col, tptr, trow, tperm)
        ctx.conf = (alpha, reg, target, fused, split_len)
        return X

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gX):
        Y, G, X, val, rowptr, col, tptr, trow, tperm = ctx.saved_tensors
        alpha, reg, target, fused, split_len = ctx.conf
        csr = (rowptr, col) if val is None else (rowptr, col, val)
        tr = None if tptr is None else (tptr, trow, tperm)
        want = val is not None and ctx.needs_input_grad[1]
        gX = gX.contiguous()
        if fused:
            dY, dval = als_adjoint_kernel(Y, G, csr, X, gX, alpha, reg, target, tr, want, split_len, None, check_range=False)
        else:
            dY, dval = als_adjoint_composed(Y, G, csr, X, gX, alpha, reg, target, tr, want)
        return (dY, dval) + (None,) * 10


def als_solve(Y, csr, alpha, reg, target='relaxed', route='auto', transposed=None, split_len=None):
    """X = the row solve of every CSR row given Y, once differentiable in Y and in the CSR's val (when the CSR has one).  G = gram(Y) is computed
    inside and its path is part of the gradient.  An unrolled ALS sweep is two calls: the second with the first's result as Y and the transposed CSR.
    route as in als_adjoint (one route serves the forward and the backward); transposed: the by-column order for the backward, built on first use
    when None.  A row subset is not offered: a repeated row would give dval two writers."""
    what = 'als_solve'
    _route(route, what)
    _target(target, what)
    n, d = als._table(Y, what)
    rowptr, col, val = als._csr(csr, what)
    alpha, reg = als._coefs(alpha, reg, what)
    n_rows, nnz = rowptr.numel() - 1, col.numel()
    fused = _pick(route, Y, n_rows, nnz) == 'fused'
    if fused:                                          # everything als_solve_rows_target and als_adjoint_kernel would refuse, before any launch
        o = _ops()
        o._dev(Y.detach().contiguous(), torch.float32, 'Y', 2)
        if not als.als_supported(d, n, n_rows, nnz):
            raise ValueError('%s: n = %d, n_rows = %d, d = %d outside the kernel\'s limits (d in %s, rows <= %d, nnz < 2^31): use the composed route'
                             % (what, n, n_rows, d, als.ALS_WIDTHS, als.ALS_MAX_ROWS))
        o._dev(rowptr, torch.int32, 'csr rowptr', 1); o._dev(col, torch.int32, 'csr col', 1)
        if val is not None:
            o._dev(val.detach(), torch.float32, 'csr val', 1)
        _split(split_len, what)
        als._check_range(rowptr, col, None, n, what)
    tptr, trow, tperm = (None, None, None) if (transposed is None and nnz == 0) else _transposed(transposed, rowptr, col, n_rows, n, what, True)
    return _AlsSolve.apply(Y, val, rowptr, col, tptr, trow, tperm, alpha, reg, target, fused, split_len)

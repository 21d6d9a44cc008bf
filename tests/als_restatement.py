"""Float64 numpy restatement of alternating least squares for implicit feedback (Hu, Koren, Volinsky, ICDM'08) -- not a test.  It states what
arlib_amd/als.py and recommender/iALS.py compute, from the definitions alone: the Gram matrix, the row update by a dense solve per row, the objective
as the dense sum over ALL pairs (and by the Gram identity), and a sweep.

    L   = sum_u sum_i c_ui (p_ui - x_u . y_i)^2 + reg (|X|^2 + |Y|^2),   p = 1 on the stored entries, c = 1 + alpha w there and 1 elsewhere
    A_r = G + alpha sum_{i in P_r} w_ri y_i y_i^T + reg I,   b_r = sum_{i in P_r} (1 + alpha w_ri) y_i,   x_r = A_r^-1 b_r,   G = Y^T Y"""
import numpy as np


def f64(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def ints(a):
    if hasattr(a, 'detach'):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.int64)


def gram(Y):
    Y = f64(Y)
    return Y.T @ Y


def solve_rows(Y, rowptr, col, val, alpha, reg, rows=None):
    """x_r of the listed CSR rows (all rows without `rows`), each by one dense solve; a row without entries is 0."""
    Y, rowptr, col = f64(Y), ints(rowptr), ints(col)
    w_all = np.ones(len(col)) if val is None else f64(val)
    G, d = gram(Y), Y.shape[1]
    sel = np.arange(len(rowptr) - 1) if rows is None else ints(rows)
    X = np.zeros((len(sel), d))
    for j, r in enumerate(sel):
        lo, hi = rowptr[r], rowptr[r + 1]
        if hi == lo:
            continue
        Yr, w = Y[col[lo:hi]], w_all[lo:hi]
        A = G + alpha * (Yr.T * w) @ Yr + reg * np.eye(d)
        b = ((1.0 + alpha * w)[:, None] * Yr).sum(0)
        X[j] = np.linalg.solve(A, b)
    return X


def dense(rowptr, col, val, n_rows, n):
    """(P [n_rows, n] 0/1, W [n_rows, n] the weights on the stored entries)."""
    rowptr, col = ints(rowptr), ints(col)
    r = np.repeat(np.arange(n_rows), np.diff(rowptr))
    P, W = np.zeros((n_rows, n)), np.zeros((n_rows, n))
    P[r, col] = 1.0
    W[r, col] = 1.0 if val is None else f64(val)
    return P, W


def dense_objective(X, Y, rowptr, col, val, alpha, reg):
    """L as the sum over every pair of the score matrix."""
    X, Y = f64(X), f64(Y)
    P, W = dense(rowptr, col, val, X.shape[0], Y.shape[0])
    S = X @ Y.T
    return float(((1.0 + alpha * W) * (P - S) ** 2).sum() + reg * ((X * X).sum() + (Y * Y).sum()))


def gram_objective(X, Y, rowptr, col, val, alpha, reg):
    """L by the Gram identity: sum_i (x . y_i)^2 = x^T G x."""
    X, Y, rowptr, col = f64(X), f64(Y), ints(rowptr), ints(col)
    w = np.ones(len(col)) if val is None else f64(val)
    r = np.repeat(np.arange(X.shape[0]), np.diff(rowptr))
    s = (X[r] * Y[col]).sum(1)
    return float(((X @ gram(Y)) * X).sum() + ((1.0 + alpha * w) * (1.0 - s) ** 2 - s * s).sum() + reg * ((X * X).sum() + (Y * Y).sum()))


def transpose(rowptr, col, val, n_rows, n):
    """The by-column CSR of a by-row CSR, a column's entries in ascending row order."""
    rowptr, col = ints(rowptr), ints(col)
    r = np.repeat(np.arange(n_rows), np.diff(rowptr))
    order = np.argsort(col, kind='stable')
    tptr = np.zeros(n + 1, np.int64)
    tptr[1:] = np.cumsum(np.bincount(col, minlength=n))
    return tptr, r[order], None if val is None else f64(val)[order]


def sweep(X, Y, rowptr, col, val, alpha, reg, halves=2, trace=None):
    """`halves` half-sweeps from the user side on: all user rows given Y, then all item rows given the new X, ...  trace, a list, receives the
    dense objective after each half-sweep."""
    X, Y = f64(X).copy(), f64(Y).copy()
    tptr, tcol, tval = transpose(rowptr, col, val, X.shape[0], Y.shape[0])
    for h in range(halves):
        if h % 2 == 0:
            X = solve_rows(Y, rowptr, col, val, alpha, reg)
        else:
            Y = solve_rows(X, tptr, tcol, tval, alpha, reg)
        if trace is not None:
            trace.append(dense_objective(X, Y, rowptr, col, val, alpha, reg))
    return X, Y

"""Every kernel entry at every embedding-width class, against float64 written here.

The SpMM family maps one row onto LPR = 4 / 8 / 16 / 32 / 64 lanes for d <= 16 / 32 / 64 / 128 / 256; a width that does not fill its class
leaves lanes masked by the `q * 4 < d` guards (plain rows, long-row partials, flag-mask windows, epilogues).  WIDTHS holds every class twice,
once full and once ragged.  Entries without a width limit also run at d = 1, 3, 65, 257, 300.  The bar is conftest.close() (max-norm AND
row-wise), so a wrong tail lane of a small row fails.  Each entry's first rejected width on each side must raise ValueError in `ops` before
any launch, and the raw C entry, called with valid device pointers, must return ARL_E_DIM."""
import ctypes as C
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from conftest import close

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
WIDTHS = (4, 12, 16, 20, 32, 36, 64, 100, 128, 132, 252, 256)
FREE_WIDTHS = WIDTHS + (1, 3, 65, 257, 300)            # entries with no width limit
ROW_COUNTS = (1, 15, 16, 17, 63, 64, 65, 257)
ARL_E_DIM = -2
TOL = 1e-5                                             # single kernels against float64
TOL_EW = 1e-6                                          # element-wise kernels


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on the MI355X box)')
    from arlib_amd import ops as _ops
    return _ops


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def H(t):
    return t.detach().cpu().numpy().astype(np.float64)


def P(t):
    return C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _clib():
    from arlib_amd import _lib
    return _lib.lib()


def bipartite(seed, U=300, I=80, hot=2, hot_deg=150):
    """Bipartite normalised adjacency with empty user rows and a few hot items whose rows take the chunked long-row plan (chunk = 32)."""
    from test_gpu_kernels import random_graph, make_csr
    rng = np.random.default_rng(seed)
    u, i = random_graph(rng, U, I, 6, hot_items=hot, hot_deg=hot_deg, empty_users=(3, 17, 101))
    rowptr, col, _, val = make_csr(u, i, U, I)
    deg = np.diff(rowptr)
    assert deg.min() == 0 and deg.max() > 4 * 32                # empty rows and long rows present
    return U, I, rowptr, col, val


def sp64(rowptr, col, val, n_cols=None):
    n = len(rowptr) - 1
    return sp.csr_matrix((val.astype(np.float64), col.astype(np.int64), rowptr.astype(np.int64)), shape=(n, n if n_cols is None else n_cols))


def graph(ops, rowptr, col, val, chunk=32):
    A = ops.CSRGraph(rowptr, col, val, DEV, chunk=chunk)
    assert A.n_long > 0
    return A


def adam64(Pm, g, M, V, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    M = b1 * M + (1 - b1) * g
    V = b2 * V + (1 - b2) * g * g
    denom = np.sqrt(V) / np.sqrt(1 - b2 ** step) + eps
    return Pm - lr / (1 - b1 ** step) * M / denom, M, V


def adam_state(rng, N, d):
    return ((rng.standard_normal((N, d)) * 0.1).astype(np.float32), (rng.standard_normal((N, d)) * 0.01).astype(np.float32),
            (rng.random((N, d)) * 1e-4).astype(np.float32))


def check_adam(Pt, Mt, Vt, P0, M0, V0, g, lr, step):
    Pr, Mr, Vr = adam64(P0.astype(np.float64), g, M0.astype(np.float64), V0.astype(np.float64), lr, step)
    assert close(H(Mt), Mr, tol=TOL) and close(H(Vt), Vr, tol=TOL)
    assert close(H(Pt), Pr, tol=TOL)
    assert close(H(Pt) - P0, Pr - P0, tol=1e-4)          # the update itself: fp32 cancellation of |P| ~ 0.1 against lr-sized steps costs ~1e-6


# ------------------------------------------------------------------------------------------------ SpMM, CSR schedule
@pytest.mark.parametrize('d', WIDTHS)
def test_spmm_csr_epilogues(ops, d):
    U, I, rowptr, col, val = bipartite(d)
    N = U + I
    A, A64 = graph(ops, rowptr, col, val), sp64(rowptr, col, val)
    rng = np.random.default_rng(100 + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    Z = rng.standard_normal((N, d)).astype(np.float32)
    rs = (rng.random(N) * 2 - 0.5).astype(np.float32)
    AX = A64 @ X.astype(np.float64)
    assert close(H(ops.spmm(A, T(X))), AX, tol=TOL)
    assert close(H(ops.spmm(A, T(X), 0.25, -1.5, T(Z))), 0.25 * AX - 1.5 * Z, tol=TOL)
    assert close(H(ops.spmm(A, T(X), row_scale=T(rs))), rs[:, None] * AX, tol=TOL)
    assert close(H(ops.spmm(A, T(X), 0.5, 2.0, T(Z), row_scale=T(rs))), 0.5 * rs[:, None] * AX + 2.0 * Z, tol=TOL)
    S, Y = T(Z.copy()), torch.empty(N, d, device=DEV)
    ops.spmm_layersum(A, T(X), T(Z), S, Y)
    assert close(H(Y), AX, tol=TOL) and close(H(S), Z + AX, tol=TOL)
    S2 = T(Z.copy())
    ops.spmm_layersum(A, T(X), S2, S2)                            # in place, no Y
    assert close(H(S2), Z + AX, tol=TOL)


@pytest.mark.parametrize('d', (4, 20, 252, 256))
@pytest.mark.parametrize('n', ROW_COUNTS)
def test_spmm_row_counts_on_wave_edges(ops, n, d):
    """Square graphs with 1 .. 257 rows (empty rows, rows through the chunk plan) at the narrowest and widest classes."""
    rng = np.random.default_rng(n * 1000 + d)
    M = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, format='lil', dtype=np.float64)
    M[0, :] = 0
    M[n - 1, :] = rng.random(n) + 0.1                            # the last row is the longest (> chunk when n > 8)
    M = M.tocsr().astype(np.float32)
    M.sort_indices()
    rowptr, col, val = M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data.astype(np.float32)
    A = ops.CSRGraph(rowptr, col, val, DEV, chunk=8)
    X = rng.standard_normal((n, d)).astype(np.float32)
    Z = rng.standard_normal((n, d)).astype(np.float32)
    AX = sp64(rowptr, col, val) @ X.astype(np.float64)
    assert close(H(ops.spmm(A, T(X), 1.0, 0.5, T(Z))), AX + 0.5 * Z, tol=TOL)


@pytest.mark.parametrize('d', WIDTHS)
def test_spmm_rows_subset(ops, d):
    U, I, rowptr, col, val = bipartite(d + 1)
    N = U + I
    A, A64 = graph(ops, rowptr, col, val), sp64(rowptr, col, val)
    rng = np.random.default_rng(200 + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    L1, L2 = (rng.standard_normal((N, d)).astype(np.float32) for _ in range(2))
    AX = A64 @ X.astype(np.float64)
    hot = np.argsort(np.diff(rowptr))[-3:]
    rows = np.concatenate([rng.integers(0, N, 60), hot, hot, [3, 3, 17, N - 1, 0]]).astype(np.int32)      # duplicates, long rows, empty rows
    w = rng.random(len(rows)).astype(np.float32)
    for nsplit in (1, 16):
        out = ops.spmm_rows(A, T(X), T(rows), (), 1.0, nsplit=nsplit)
        assert close(H(out), AX[rows], tol=TOL)
        out = ops.spmm_rows(A, T(X), T(rows), (T(L1), T(L2)), 0.25, nsplit=nsplit, row_weight=T(w))
        assert close(H(out), 0.25 * w[:, None] * (L1[rows] + L2[rows] + AX[rows]), tol=TOL)


@pytest.mark.parametrize('d', WIDTHS)
def test_spmm_flagged_masked_order(ops, d):
    U, I, rowptr, col, val = bipartite(d + 2)
    N = U + I
    A, A64 = graph(ops, rowptr, col, val).enable_masked_order(), sp64(rowptr, col, val)
    rng = np.random.default_rng(300 + d)
    flag = rng.random(N) < 0.2
    flag[np.argsort(np.diff(rowptr))[-2:]] = True               # long rows flagged too
    X = (rng.standard_normal((N, d)) * flag[:, None]).astype(np.float32)      # the bitmap form's contract: X is zero off the flagged rows
    Z = rng.standard_normal((N, d)).astype(np.float32)
    zf = (rng.random(N) < 0.3).astype(np.uint8)
    Zs = Z * zf[:, None]
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    ops.mark_bits_(bits, T(np.nonzero(flag)[0].astype(np.int32)), True, N)
    AX = A64 @ X.astype(np.float64)
    assert close(H(ops.spmm_flagged(A, T(X), bits)), AX, tol=TOL)
    assert close(H(ops.spmm_flagged(A, T(X), bits, 0.5, 2.0, T(Zs), T(zf))), 0.5 * AX + 2.0 * Zs, tol=TOL)
    assert close(H(ops.spmm_flagged(A, T(X), None, 0.5, 2.0, T(Zs), T(zf))), 0.5 * AX + 2.0 * Zs, tol=TOL)
    assert close(H(ops.spmm_flagged(A, T(X), None, 1.0, -1.0, T(Z))), AX - Z, tol=TOL)


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('use_zflags', [False, True])
def test_spmm_adam_epilogue(ops, d, use_zflags):
    U, I, rowptr, col, val = bipartite(d + 3)
    N = U + I
    A, A64 = graph(ops, rowptr, col, val), sp64(rowptr, col, val)
    rng = np.random.default_rng(400 + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    Z = rng.standard_normal((N, d)).astype(np.float32)
    zf = (rng.random(N) < 0.3).astype(np.uint8)
    if use_zflags:
        Z = Z * zf[:, None]
    P0, M0, V0 = adam_state(rng, N, d)
    Pt, Mt, Vt = T(P0), T(M0), T(V0)
    ops.spmm_adam(A, T(X), 0.25, 0.5, T(Z), Pt, Mt, Vt, 0.005, 7, zflags=T(zf) if use_zflags else None)
    g = 0.25 * (A64 @ X.astype(np.float64)) + 0.5 * Z
    check_adam(Pt, Mt, Vt, P0, M0, V0, g, 0.005, 7)


# ------------------------------------------------------------------------------------------------ SpMM, blocked schedule
@pytest.mark.parametrize('d', WIDTHS)
def test_spmm_blocked_schedule_or_csr_fallback(ops, d, monkeypatch):
    """A graph with a register-blocked plan: d = 64 and 128 run through it, every other width keeps the CSR kernel; the numbers hold both ways."""
    U, I, rowptr, col, val = bipartite(d + 5, U=700, I=150, hot=3, hot_deg=400)
    N = U + I
    A, A64 = graph(ops, rowptr, col, val), sp64(rowptr, col, val)
    A.enable_blocked(split=U, rows_per_wave=16, hub=64, col_block=256)
    calls = []
    real = A.blocked.struct
    monkeypatch.setattr(A.blocked, 'struct', lambda k, dd: (calls.append(dd), real(k, dd))[1])
    rng = np.random.default_rng(600 + d)
    X = rng.standard_normal((N, d)).astype(np.float32)
    Z = rng.standard_normal((N, d)).astype(np.float32)
    AX = A64 @ X.astype(np.float64)
    assert close(H(ops.spmm(A, T(X), 0.5, 2.0, T(Z))), 0.5 * AX + 2.0 * Z, tol=TOL)
    S, Y = T(Z.copy()), torch.empty(N, d, device=DEV)
    ops.spmm_layersum(A, T(X), S, S, Y)
    assert close(H(Y), AX, tol=TOL) and close(H(S), Z + AX, tol=TOL)
    P0, M0, V0 = adam_state(rng, N, d)
    Pt, Mt, Vt = T(P0), T(M0), T(V0)
    ops.spmm_adam(A, T(X), 0.25, 0.5, T(Z), Pt, Mt, Vt, 0.005, 2)
    check_adam(Pt, Mt, Vt, P0, M0, V0, 0.25 * AX + 0.5 * Z, 0.005, 2)
    if d in (64, 128):
        assert calls and set(calls) == {d}
    else:
        assert calls == []


# ------------------------------------------------------------------------------------------------ SDDMM
@pytest.mark.parametrize('d', WIDTHS)
def test_sddmm_csr(ops, d):
    U, I, rowptr, col, val = bipartite(d + 6)
    N = U + I
    A = graph(ops, rowptr, col, val)
    rng = np.random.default_rng(700 + d)
    dY = rng.standard_normal((N, d)).astype(np.float32)
    X = rng.standard_normal((N, d)).astype(np.float32)
    erow = np.repeat(np.arange(N), np.diff(rowptr))
    a, b = dY[erow].astype(np.float64), X[col].astype(np.float64)
    ref = 0.75 * np.einsum('ij,ij->i', a, b)
    # one output per edge, each a single dot product: held to 1e-5 of its own conditioning 0.75 ||dY_row|| ||X_col|| (a dot product that
    # cancels to ~0 has no relative accuracy in fp32), plus the max-norm bar
    cond = 0.75 * np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)
    out = H(ops.sddmm_csr(A, T(dY), T(X), 0.75))
    assert np.all(np.abs(out - ref) <= TOL * cond) and close(out, ref, tol=TOL, row_tol=np.inf)
    base = rng.standard_normal(len(col)).astype(np.float32)
    out = H(ops.sddmm_csr(A, T(dY), T(X), 0.75, out=T(base)))             # accumulates
    assert np.all(np.abs(out - base - ref) <= TOL * (cond + np.abs(base))) and close(out, base + ref, tol=TOL, row_tol=np.inf)


@pytest.mark.parametrize('d', WIDTHS + (1, 3, 65))
def test_sddmm_rows_dense(ops, d):
    rng = np.random.default_rng(800 + d)
    n, Nx, off, nc = 90, 400, 37, 333
    dY = rng.standard_normal((n, d)).astype(np.float32)
    X = rng.standard_normal((Nx, d)).astype(np.float32)
    rows = np.array([0, 5, 5, 89, 17, 63, 64, 65], np.int32)
    ref = dY[rows].astype(np.float64) @ X[off:off + nc].astype(np.float64).T
    assert close(H(ops.sddmm_rows_dense(T(dY), T(X), T(rows), off, nc)), ref, tol=TOL)


# ------------------------------------------------------------------------------------------------ losses
BATCHES = (1, 63, 64, 65, 2048)


def loss_batch(B, U, I, seed):
    rng = np.random.default_rng(seed)
    u, p, n = rng.integers(0, U, B), rng.integers(0, I, B), rng.integers(0, I, B)
    if B > 1:
        u[: B // 3] = u[0]                                   # one user owns a third of the batch
        n[1::7] = p[0]                                       # item p[0] is both a positive (sample 0) and a negative (samples 1, 8, ...)
        p[2::11] = p[0]
    else:
        n[0] = (p[0] + 1) % I                                # p = n in one sample cancels its bpr gradient to fp32 noise
    return u.astype(np.int32), p.astype(np.int32), n.astype(np.int32)


def bpr64(E, off, u, p, n, reg, upstream=1.0):
    Et = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    ue, pe, ne = Et[torch.from_numpy(u.astype(np.int64))], Et[off + torch.from_numpy(p.astype(np.int64))], Et[off + torch.from_numpy(n.astype(np.int64))]
    x = (ue * pe).sum(1) - (ue * ne).sum(1)
    bpr = (-torch.log(1e-7 + torch.sigmoid(x))).mean()
    nu, npn = torch.norm(ue), torch.norm(pe)
    (upstream * (bpr + reg * (nu + npn))).backward()
    return np.array([bpr.item(), reg * (nu + npn).item(), nu.item(), npn.item()]), Et.grad.numpy()


def wrmf64(E, off, u, p, n, reg, w, upstream=1.0):
    Et = torch.tensor(E, dtype=torch.float64, requires_grad=True)
    ue, pe, ne = Et[torch.from_numpy(u.astype(np.int64))], Et[off + torch.from_numpy(p.astype(np.int64))], Et[off + torch.from_numpy(n.astype(np.int64))]
    lw = (w * ((ue * pe).sum(1) - 1) ** 2 + (ue * ne).sum(1) ** 2).sum()
    nu, npn = torch.norm(ue), torch.norm(pe)
    (upstream * (lw + reg * (nu + npn))).backward()
    return np.array([lw.item(), reg * (nu + npn).item(), nu.item(), npn.item()]), Et.grad.numpy()


def loss_close(got, ref, tol=TOL):
    return all(abs(g - r) <= tol * max(abs(r), 1e-30) for g, r in zip(got, ref))


@pytest.mark.parametrize('d', FREE_WIDTHS)
@pytest.mark.parametrize('B', BATCHES)
def test_bpr_l2_fwd_bwd(ops, d, B):
    U, I = 300, 200
    rng = np.random.default_rng(900 + d + B)
    E = (rng.standard_normal((U + I, d)) * 0.3).astype(np.float32)
    u, p, n = loss_batch(B, U, I, d * 7 + B)
    ref, gref = bpr64(E, U, u, p, n, 1e-2, upstream=0.5)
    Gs = []
    for _ in range(2):
        G = torch.zeros(U + I, d, device=DEV)
        lo = ops.bpr_l2_fwd_bwd(T(E), U, T(u), T(p), T(n), 1e-2, G, upstream=0.5)
        Gs.append(G)
    assert loss_close(H(lo), ref), (H(lo), ref)
    assert close(H(Gs[0]), gref, tol=TOL)
    assert torch.equal(Gs[0], Gs[1])                                    # bit for bit across calls


@pytest.mark.parametrize('d', FREE_WIDTHS)
@pytest.mark.parametrize('B', (63, 2048))
def test_bpr_l2_sharded_pair(ops, d, B):
    """bpr_l2_partial on two halves of a batch + the caller's reduction + bpr_l2_backward of each half = the whole batch's loss and gradient."""
    U, I = 300, 200
    rng = np.random.default_rng(1000 + d + B)
    E = (rng.standard_normal((U + I, d)) * 0.3).astype(np.float32)
    u, p, n = loss_batch(B, U, I, d * 5 + B)
    reg = 1e-2
    ref, gref = bpr64(E, U, u, p, n, reg)
    h = B // 2 + 1
    parts = [(T(u[a:b]), T(p[a:b]), T(n[a:b])) for a, b in ((0, h), (h, B))]
    wss = [torch.zeros(4 * max(b.numel(), 1), device=DEV) for b, _, _ in parts]
    sums = torch.zeros(3, device=DEV)
    for (bu, bp, bn), ws in zip(parts, wss):
        sums += ops.bpr_l2_partial(T(E), U, bu, bp, bn, B, ws, torch.zeros(3, device=DEV))
    nu, npn = torch.sqrt(sums[1]), torch.sqrt(sums[2])
    norms4 = torch.stack([sums[0] / B, reg * (nu + npn), nu, npn]).contiguous()
    assert loss_close(H(norms4), ref)
    G = torch.zeros(U + I, d, device=DEV)
    for (bu, bp, bn), ws in zip(parts, wss):
        ops.bpr_l2_backward(T(E), U, bu, bp, bn, reg, norms4, G, ws)
    assert close(H(G), gref, tol=TOL)


@pytest.mark.parametrize('d', FREE_WIDTHS)
@pytest.mark.parametrize('B', BATCHES)
def test_wrmf_l2_fwd_bwd(ops, d, B):
    U, I = 300, 200
    rng = np.random.default_rng(1100 + d + B)
    E = (rng.standard_normal((U + I, d)) * (0.6 / np.sqrt(d))).astype(np.float32)
    u, p, n = loss_batch(B, U, I, d * 3 + B)
    ref, gref = wrmf64(E, U, u, p, n, 1e-2, 20.0, upstream=0.5)
    Gs = []
    for _ in range(2):
        G = torch.zeros(U + I, d, device=DEV)
        lo = ops.wrmf_l2_fwd_bwd(T(E), U, T(u), T(p), T(n), 1e-2, 20.0, G, upstream=0.5)
        Gs.append(G)
    assert loss_close(H(lo), ref), (H(lo), ref)
    assert close(H(Gs[0]), gref, tol=TOL)
    assert torch.equal(Gs[0], Gs[1])


# ------------------------------------------------------------------------------------------------ SimGCL pieces
def infonce64(v1, v2, tau, upstream):
    a = torch.tensor(v1, dtype=torch.float64, requires_grad=True)
    b = torch.tensor(v2, dtype=torch.float64, requires_grad=True)
    an, bn = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(b, dim=1)
    logits = an @ bn.T / tau
    loss = (torch.logsumexp(logits, 1) - logits.diagonal()).mean()
    (upstream * loss).backward()
    return loss.item(), a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('n', (1, 63, 64, 65, 257))
def test_infonce_fwd_bwd(ops, d, n):
    rng = np.random.default_rng(1200 + d + n)
    v1 = rng.standard_normal((n, d)).astype(np.float32)
    v2 = (v1 + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ref, g1, g2 = infonce64(v1, v2, 0.2, 0.7)
    loss, d1, d2 = ops.infonce_fwd_bwd(T(v1), T(v2), 0.2, upstream=0.7)
    assert abs(loss.item() - ref) <= TOL * max(abs(ref), 1.0)          # n = 1: the loss is 0
    assert close(H(d1), g1, tol=TOL) and close(H(d2), g2, tol=TOL)


@pytest.mark.parametrize('d', (12, 256))
def test_infonce_at_its_row_limit(ops, d):
    n = 8192
    rng = np.random.default_rng(1300 + d)
    v1 = rng.standard_normal((n, d)).astype(np.float32)
    v2 = (v1 + 0.5 * rng.standard_normal((n, d))).astype(np.float32)
    ref, g1, g2 = infonce64(v1, v2, 0.2, 1.0)
    loss, d1, d2 = ops.infonce_fwd_bwd(T(v1), T(v2), 0.2)
    assert abs(loss.item() - ref) <= TOL * abs(ref)
    # each gradient entry sums 8192 softmax-weighted terms that cancel to ~1e-6 (the 1/n mean), and the fp32 logits carry ~sqrt(d) eps / tau of
    # absolute error: measured against float64 at d = 256 the max-norm error is 1.5e-5 (row-wise 6.6e-6), so the max-norm bar is 3e-5 here
    assert close(H(d1), g1, tol=3e-5, row_tol=TOL) and close(H(d2), g2, tol=3e-5, row_tol=TOL)
    with pytest.raises(ValueError):
        ops.infonce_fwd_bwd(torch.zeros(n + 1, d, device=DEV), torch.zeros(n + 1, d, device=DEV), 0.2)


@pytest.mark.parametrize('d', FREE_WIDTHS)
def test_simgcl_perturb(ops, d):
    rng = np.random.default_rng(1400 + d)
    n = 257
    E = rng.standard_normal((n, d)).astype(np.float32)
    E[::5, 0] = 0.0                                             # sign(0) = 0: no noise on that entry
    noise = rng.random((n, d)).astype(np.float32)
    noise[7] = 0.0                                              # a zero noise row stays zero (F.normalize's 1e-12 floor)
    E64, N64 = E.astype(np.float64), noise.astype(np.float64)
    nn_ = N64 / np.maximum(np.linalg.norm(N64, axis=1, keepdims=True), 1e-12)
    ref = E64 + np.sign(E64) * nn_ * 0.1
    out = ops.simgcl_perturb_(T(E), T(noise), 0.1)
    assert close(H(out), ref, tol=TOL_EW)


@pytest.mark.parametrize('d', (1, 3) + WIDTHS)
def test_simgcl_perturb_rng_row_norms(ops, d):
    """The in-kernel noise: non-negative, one unit direction per row, so every row moves by exactly eps along sign(E)."""
    rng = np.random.default_rng(1500 + d)
    n = 257
    E = (rng.standard_normal((n, d)) + 0.01).astype(np.float32)
    E = np.where(np.abs(E) < 1e-3, 0.5, E).astype(np.float32)
    out = H(ops.simgcl_perturb_rng(T(E), 0.1, 11, 3))
    delta = (out - E.astype(np.float64)) * np.sign(E)
    assert delta.min() >= -1e-6
    assert np.allclose(np.linalg.norm(delta, axis=1), 0.1, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ row utilities
@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('n', (1, 17, 65, 257))
def test_normalize_rows_and_bwd(ops, d, n):
    rng = np.random.default_rng(1600 + d + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[n // 2] = 0.0                                             # zero row: 1e-12 floor
    dY = rng.standard_normal((n, d)).astype(np.float32)
    X64 = X.astype(np.float64)
    nrm = np.maximum(np.linalg.norm(X64, axis=1), 1e-12)
    Y64 = X64 / nrm[:, None]
    Y, nr = ops.normalize_rows(T(X))
    assert close(H(Y), Y64, tol=TOL) and close(H(nr), nrm, tol=TOL)
    Yc = Y.clone()
    dX = ops.normalize_rows_bwd(Yc, nr, T(dY), 0.5)
    Yh = H(Yc)                                                  # the kernel's own Y: the backward is held to float64 of its inputs
    ref = 0.5 * (dY - Yh * (Yh * dY).sum(1, keepdims=True)) / H(nr)[:, None]
    assert close(H(dX), ref, tol=TOL)


@pytest.mark.parametrize('d', FREE_WIDTHS)
@pytest.mark.parametrize('n', ROW_COUNTS)
def test_gather_scatter_axpy_zero_rows(ops, d, n):
    rng = np.random.default_rng(1700 + d + n)
    N = 300
    src = rng.standard_normal((N, d)).astype(np.float32)
    idx = rng.integers(0, N, n).astype(np.int32)
    idx[: n // 3] = idx[0]                                     # duplicates
    assert torch.equal(ops.gather_rows(T(src), T(idx)).cpu(), torch.from_numpy(src[idx]))
    add = rng.standard_normal((n, d)).astype(np.float32)
    ref = src.astype(np.float64).copy()
    np.add.at(ref, idx, 0.5 * add.astype(np.float64))
    assert close(H(ops.scatter_add_rows(T(src), T(idx), T(add), 0.5)), ref, tol=TOL)
    table = np.zeros((N, d), np.float32)
    table[idx] = rng.standard_normal((n, d)).astype(np.float32)[: len(idx)]
    ref = src.astype(np.float64).copy()
    uniq = np.unique(idx)
    ref[uniq] += -1.5 * table[uniq].astype(np.float64)
    assert close(H(ops.rows_axpy_unique_(T(src), T(table), T(idx), -1.5)), ref, tol=TOL_EW)
    ref = src.copy()
    ref[idx] = 0.0
    assert torch.equal(ops.zero_rows_(T(src), T(idx)).cpu(), torch.from_numpy(ref))


@pytest.mark.parametrize('d', FREE_WIDTHS)
def test_batch_rows_set_and_clear(ops, d):
    rng = np.random.default_rng(1800 + d)
    N, n = 300, 65
    G0 = rng.standard_normal((N, d)).astype(np.float32)
    idx = rng.integers(0, N, n).astype(np.int32)
    idx[:20] = idx[0]; idx[40:45] = idx[1]
    src = rng.standard_normal((n, d)).astype(np.float32)
    rs = rng.random(n).astype(np.float32)
    for dup in (False, True):
        G, flags = T(G0), torch.zeros(N, dtype=torch.uint8, device=DEV)
        bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
        db = torch.zeros_like(bits) if dup else None
        ops.batch_rows_set_(G, flags, bits, T(idx), T(src), 0.5, row_scale=T(rs), dup_bits=db)
        ref = G0.astype(np.float64).copy()
        np.add.at(ref, idx, 0.5 * rs[:, None].astype(np.float64) * src)
        assert close(H(G), ref, tol=TOL)
        want = np.zeros(N, bool); want[idx] = True
        assert np.array_equal(flags.cpu().numpy() != 0, want)
        b = bits.cpu().numpy().view(np.uint32)
        assert np.array_equal(((b[np.arange(N) >> 5] >> (np.arange(N) & 31)) & 1) != 0, want)
        ops.batch_rows_clear_(G, flags, bits, T(idx), dup_bits=db)
        ref[idx] = 0.0
        assert close(H(G), ref, tol=TOL) and int(flags.max()) == 0 and int(bits.abs().max()) == 0
        if db is not None:
            assert int(db.abs().max()) == 0


@pytest.mark.parametrize('d', WIDTHS + (300,))
def test_tables_sum(ops, d):
    rng = np.random.default_rng(1900 + d)
    tabs = [rng.standard_normal((65, d)).astype(np.float32) for _ in range(5)]
    for k in (1, 3, 5):
        out = ops.tables_sum([T(t) for t in tabs[:k]], 0.25)
        assert close(H(out), 0.25 * sum(t.astype(np.float64) for t in tabs[:k]), tol=TOL_EW)


# ------------------------------------------------------------------------------------------------ NGCF element-wise kernels
def _with_zeros(rng, n, d):
    Z = rng.standard_normal((n, d)).astype(np.float32)
    Z[rng.random((n, d)) < 0.1] = 0.0                          # exact zeros: torch takes the negative-side slope there
    Z[:, -1] = 0.0                                             # ... in the last lane of every row too
    return Z


@pytest.mark.parametrize('d', WIDTHS + (300,))
@pytest.mark.parametrize('n', (1, 63, 65, 257))
def test_ngcf_elementwise_kernels(ops, d, n):
    rng = np.random.default_rng(2000 + d + n)
    Pm, E = (rng.standard_normal((n, d)).astype(np.float32) for _ in range(2))
    P64, E64 = Pm.astype(np.float64), E.astype(np.float64)
    assert close(H(ops.ngcf_combine(T(Pm), T(E))), np.concatenate([P64 + E64, P64 * E64], 1), tol=TOL_EW)
    slope = 0.01
    Z = _with_zeros(rng, n, d)
    Z64 = Z.astype(np.float64)
    act = np.where(Z64 > 0, Z64, slope * Z64)
    assert close(H(ops.ngcf_act_(T(Z), None, slope)), act, tol=TOL_EW)
    acc0 = rng.standard_normal((n, d)).astype(np.float32)
    acc = T(acc0)
    out = ops.ngcf_act_(T(Z), acc, slope)
    assert close(H(out), act, tol=TOL_EW) and close(H(acc), acc0 + act, tol=TOL_EW)
    gOut = rng.standard_normal((n, d)).astype(np.float32)
    Out = np.where(Z > 0, Z, np.float32(slope) * Z).astype(np.float32)
    ref = np.where(Out.astype(np.float64) > 0, 1.0, slope) * gOut
    assert close(H(ops.ngcf_act_bwd(T(gOut), T(Out), slope)), ref, tol=TOL_EW)
    # torch's own leaky_relu backward at the same points, zeros included
    zt = torch.tensor(Z64, requires_grad=True)
    torch.nn.functional.leaky_relu(zt, slope).backward(torch.from_numpy(gOut.astype(np.float64)))
    assert close(H(ops.ngcf_act_bwd(T(gOut), T(Out), slope)), zt.grad.numpy(), tol=TOL_EW)
    gST = rng.standard_normal((n, 2 * d)).astype(np.float32)
    gP, gE = ops.ngcf_combine_bwd(T(gST), T(Pm), T(E))
    gS, gT = gST[:, :d].astype(np.float64), gST[:, d:].astype(np.float64)
    assert close(H(gP), gS + gT * E64, tol=TOL_EW) and close(H(gE), gS + gT * P64, tol=TOL_EW)


# ------------------------------------------------------------------------------------------------ limits
def _bufs(n=64, d=264):
    return [torch.zeros(n, d, device=DEV) for _ in range(6)]     # room for the widest rejected width: nothing can be written out of bounds


@pytest.mark.parametrize('d', (2, 6, 260))
def test_spmm_family_rejects_width(ops, d):
    U, I, rowptr, col, val = bipartite(7)
    N = U + I
    A = graph(ops, rowptr, col, val).enable_masked_order()
    X, Z, Y, Pm, M, V = (torch.zeros(N, d, device=DEV) for _ in range(6))
    rows = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        ops.spmm(A, X)
    with pytest.raises(ValueError):
        ops.spmm(A, X, row_scale=torch.ones(N, device=DEV))
    with pytest.raises(ValueError):
        ops.spmm_layersum(A, X, Z, Y)
    with pytest.raises(ValueError):
        ops.spmm_adam(A, X, 1.0, 0.0, None, Pm, M, V, 0.01, 1)
    with pytest.raises(ValueError):
        ops.spmm_flagged(A, X, torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        ops.spmm_rows(A, X, rows)
    with pytest.raises(ValueError):
        ops.sddmm_csr(A, Y, X)
    # the raw entries, with valid device pointers into buffers wide enough for d = 264
    L, st = _clib(), _stream()
    Xw, Zw, Yw, Pw, Mw, Vw = (torch.zeros(N, 264, device=DEV) for _ in range(6))
    s = A._struct(264)                                          # long-row partials sized for d = 264
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    assert L.arl_spmm_csr_f32(C.byref(s), P(Xw), d, 1.0, 0.0, None, P(Yw), st) == ARL_E_DIM
    assert L.arl_spmm_csr_rscale_f32(C.byref(s), P(Xw), d, P(Zw), 1.0, 0.0, None, P(Yw), st) == ARL_E_DIM
    assert L.arl_spmm_csr_layersum_f32(C.byref(s), P(Xw), d, P(Zw), P(Zw), P(Yw), st) == ARL_E_DIM
    assert L.arl_spmm_csr_adam_f32(C.byref(s), P(Xw), d, 1.0, 0.0, None, None, P(Pw), P(Mw), P(Vw), 0.01, 0.9, 0.999, 1e-8, 1, st) == ARL_E_DIM
    assert L.arl_spmm_csr_flagged_f32(C.byref(s), P(Xw), d, P(bits), 1.0, 0.0, None, None, P(Yw), st) == ARL_E_DIM
    ws = torch.zeros(4 * 16 * 264, device=DEV)
    layers = (C.c_void_p * 1)(None)
    assert L.arl_spmm_csr_rows_f32(C.byref(s), P(Xw), d, P(rows), 4, 16, C.cast(layers, C.c_void_p), 0, 1.0, None, P(Yw), P(ws), st) == ARL_E_DIM
    gval = torch.zeros(len(col), device=DEV)
    assert L.arl_sddmm_csr_f32(P(A.rowptr), P(A.col), N, d, P(Yw), P(Xw), 1.0, P(gval), st) == ARL_E_DIM
    torch.cuda.synchronize()
    assert float(Yw.abs().max()) == 0.0 and float(gval.abs().max()) == 0.0         # nothing launched


@pytest.mark.parametrize('d', (6, 260))
def test_row_kernels_reject_width(ops, d):
    n = 64
    X, dY = torch.ones(n, d, device=DEV), torch.ones(n, d, device=DEV)
    with pytest.raises(ValueError):
        ops.normalize_rows(X)
    with pytest.raises(ValueError):
        ops.normalize_rows_bwd(X, torch.ones(n, device=DEV), dY)
    with pytest.raises(ValueError):
        ops.infonce_fwd_bwd(X, dY, 0.2)
    L, st = _clib(), _stream()
    Xw, Yw, Dw, Ow = _bufs(n)[:4]
    nrm = torch.ones(n, device=DEV)
    assert L.arl_normalize_rows_f32(P(Xw), n, d, P(Yw), P(nrm), st) == ARL_E_DIM
    assert L.arl_normalize_rows_bwd_f32(P(Xw), P(nrm), P(Dw), n, d, 1.0, None, P(Ow), st) == ARL_E_DIM
    ws = torch.zeros(max(1, L.arl_infonce_workspace_bytes(n, 264) // 4), device=DEV)
    loss = torch.zeros(1, device=DEV)
    assert L.arl_infonce_fwd_bwd_f32(P(Xw), P(Dw), n, d, 0.2, 1.0, P(loss), P(Yw), P(Ow), P(ws), st) == ARL_E_DIM
    torch.cuda.synchronize()
    assert float(Yw.abs().max()) == 0.0 and float(Ow.abs().max()) == 0.0


@pytest.mark.parametrize('d', (257, 260))
def test_widest_row_kernels_reject_width(ops, d):
    """sddmm_rows_dense and simgcl_perturb_rng take any width up to 256."""
    n = 64
    with pytest.raises(ValueError):
        ops.sddmm_rows_dense(torch.ones(n, d, device=DEV), torch.ones(n, d, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV), 0, 8)
    with pytest.raises(ValueError):
        ops.simgcl_perturb_rng(torch.ones(n, d, device=DEV), 0.1, 1, 1)
    L, st = _clib(), _stream()
    Xw, Yw, Ow = _bufs(n)[:3]
    rows = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert L.arl_sddmm_rows_dense_f32(P(Yw), P(Xw), d, P(rows), 2, 0, 8, P(Ow), st) == ARL_E_DIM
    assert L.arl_simgcl_perturb_rng_f32(P(Xw), P(Ow), n, d, None, 0.1, 1, 1, st) == ARL_E_DIM
    torch.cuda.synchronize()
    assert float(Ow.abs().max()) == 0.0


@pytest.mark.parametrize('d', (1, 2, 3, 6, 65, 257))
def test_ngcf_elementwise_kernels_reject_width(ops, d):
    n = 64
    Pm, E = torch.ones(n, d, device=DEV), torch.ones(n, d, device=DEV)
    with pytest.raises(ValueError):
        ops.ngcf_combine(Pm, E)
    with pytest.raises(ValueError):
        ops.ngcf_act_(Pm)
    with pytest.raises(ValueError):
        ops.ngcf_act_bwd(Pm, E)
    with pytest.raises(ValueError):
        ops.ngcf_combine_bwd(torch.ones(n, 2 * d, device=DEV), Pm, E)
    L, st = _clib(), _stream()
    Aw, Bw, Sw, Ow, Qw = (torch.zeros(n, 2 * 264, device=DEV) for _ in range(5))
    assert L.arl_ngcf_combine_f32(P(Aw), P(Bw), n, d, P(Sw), st) == ARL_E_DIM
    assert L.arl_ngcf_act_f32(P(Aw), P(Ow), n, d, 0.01, st) == ARL_E_DIM
    assert L.arl_ngcf_act_bwd_f32(P(Aw), P(Bw), n, d, 0.01, P(Ow), st) == ARL_E_DIM
    assert L.arl_ngcf_combine_bwd_f32(P(Sw), P(Aw), P(Bw), n, d, P(Ow), P(Qw), st) == ARL_E_DIM
    torch.cuda.synchronize()
    assert float(Sw.abs().max()) == 0.0 and float(Ow.abs().max()) == 0.0 and float(Qw.abs().max()) == 0.0


@pytest.mark.parametrize('d', (4, 252, 300))
def test_zero_rows_are_no_ops(ops, d):
    """n = 0 wherever the C entry accepts it (raw entries, valid device pointers): status 0, nothing written."""
    L, st = _clib(), _stream()
    N = 65
    X0 = torch.randn(N, 2 * d, device=DEV)
    X, Y, Z, W = X0.clone(), X0.clone(), X0.clone(), X0.clone()
    idx = torch.zeros(8, dtype=torch.int32, device=DEV)
    flags, bits = torch.zeros(N, dtype=torch.uint8, device=DEV), torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    assert L.arl_gather_rows_f32(P(X), P(idx), 0, d, P(Y), st) == 0
    assert L.arl_scatter_add_rows_f32(P(X), P(idx), 0, d, P(Y), 1.0, st) == 0
    assert L.arl_rows_axpy_unique_f32(P(X), P(Y), P(idx), 0, d, 1.0, None, st) == 0
    assert L.arl_zero_rows_f32(P(X), P(idx), 0, d, st) == 0
    assert L.arl_batch_rows_set_f32(P(X), P(flags), P(bits), P(idx), 0, d, P(Y), 1.0, None, None, st) == 0
    assert L.arl_batch_rows_clear_f32(P(X), P(flags), P(bits), P(idx), 0, d, None, st) == 0
    assert L.arl_ngcf_combine_f32(P(X), P(Y), 0, d, P(Z), st) == 0
    assert L.arl_ngcf_act_f32(P(X), P(Y), 0, d, 0.01, st) == 0
    assert L.arl_ngcf_act_bwd_f32(P(X), P(Y), 0, d, 0.01, P(Z), st) == 0
    assert L.arl_ngcf_combine_bwd_f32(P(X), P(Y), P(Z), 0, d, P(W), P(W), st) == 0
    assert L.arl_simgcl_perturb_f32(P(X), P(Y), 0, d, 0.1, st) == 0
    if d <= 256:
        nrm = torch.ones(N, device=DEV)
        assert L.arl_normalize_rows_f32(P(X), 0, d, P(Z), P(nrm), st) == 0
        assert L.arl_normalize_rows_bwd_f32(P(X), P(nrm), P(Y), 0, d, 1.0, None, P(Z), st) == 0
        assert L.arl_simgcl_perturb_rng_f32(P(X), P(Z), 0, d, None, 0.1, 1, 1, st) == 0
        assert L.arl_sddmm_rows_dense_f32(P(X), P(Y), d, P(idx), 0, 0, 8, P(Z), st) == 0
        U, I, rowptr, col, val = bipartite(9)
        A = graph(ops, rowptr, col, val)
        Xa = torch.zeros(U + I, d, device=DEV)
        s = A._struct(d)
        ws = torch.zeros(16, device=DEV)
        layers = (C.c_void_p * 1)(None)
        assert L.arl_spmm_csr_rows_f32(C.byref(s), P(Xa), d, P(idx), 0, 16, C.cast(layers, C.c_void_p), 0, 1.0, None, P(Z), P(ws), st) == 0
    torch.cuda.synchronize()
    for t in (X, Y, Z, W):
        assert torch.equal(t, X0)
    assert int(flags.max()) == 0 and int(bits.abs().max()) == 0

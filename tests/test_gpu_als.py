"""The ALS kernels (csrc/arl_als.hip) on the device against the float64 restatement (tests/als_restatement.py), on the problems of test_als_cpu.py:
every seventh row empty, one row with 4 x the usual degree, one row holding every column, ragged degrees, both parameter families, binary and
weighted, with split_len at its default, 8 and 5 (split rows, pieces of length 1, ragged last pieces) and a row subset with a repeated and an
out-of-order index.

Bar for the solved rows: the kernel's largest row-wise relative l2 error against float64 is at most FACTOR = 2 times that of the composed fp32 route
(torch bmm + fp32 Cholesky on the device) on the same inputs; the 2 is the room for a different fp32 summation order of S = sum w y y^T -- the
kernel completes, factorises and solves A in double, which should put it below 1 x.  The composed route's own error must be at most 1e-5 for the
comparison to mean anything (test_als_cpu.py measures 3e-7 to 6e-6 on the CPU).  Gram matrix and objective are double throughout: 1e-12 relative."""
import numpy as np
import pytest
import torch
import als_restatement as R
from test_als_cpu import CASES, SHAPES, problem, reference, row_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FACTOR, PRECONDITION = 2.0, 1e-5
SPLITS = (None, 8, 5)


def on_device(P):
    return dict(P, Y=P['Y'].to(DEV), csr=tuple(t.to(DEV) for t in P['csr']))


def test_the_problems_hold_what_the_cases_need():
    for rows, n, d in SHAPES:
        deg = np.diff(problem(rows, n, d)['csr'][0].numpy())
        assert deg[0] == 0 and deg[-1] == n and deg[1] == 53 and all(deg[r] == 0 for r in range(0, rows, 7))
    deg = np.diff(problem(70, 515, 64)['csr'][0].numpy())
    for split in (8, 5):
        assert (deg > split).sum() > 3 and any(l > split and l % split == 1 for l in deg) and any(l > split and 1 < l % split for l in deg)


@pytest.mark.parametrize('rows,n,d,family,weighted', CASES)
def test_rows_against_float64_and_the_composed_route(rows, n, d, family, weighted):
    from arlib_amd import als
    Ph, want = reference(rows, n, d, family, weighted)
    P = on_device(Ph)
    G = als.gram(P['Y'])
    ec = row_err(als.als_solve_rows_composed(P['Y'], G, P['csr'], P['alpha'], P['reg']), want)
    assert ec <= PRECONDITION, ec
    base = None
    for split in SPLITS:
        got = als.als_solve_rows_kernel(P['Y'], G, P['csr'], P['alpha'], P['reg'], split_len=split)
        ek = row_err(got, want)
        print('als rows %s split_len %s: kernel %.3e composed %.3e' % ((rows, n, d, family, weighted), split, ek, ec))
        assert ek <= FACTOR * ec, (split, ek, ec)
        assert not bool(got[::7].any())                                # the empty rows are exactly 0
        assert torch.equal(got, als.als_solve_rows_kernel(P['Y'], G, P['csr'], P['alpha'], P['reg'], split_len=split))          # run to run: the same bits
        if split is None:
            base = got
    # a split_len that splits nothing gives the default's bits
    assert torch.equal(base, als.als_solve_rows_kernel(P['Y'], G, P['csr'], P['alpha'], P['reg'], split_len=n + 1))
    # a subset with a repeated and an out-of-order index, split and unsplit
    sub = torch.tensor([rows - 1, 1, 1, 0, 2], dtype=torch.int32, device=DEV)
    for split in SPLITS:
        gs = als.als_solve_rows_kernel(P['Y'], G, P['csr'], P['alpha'], P['reg'], rows=sub, split_len=split)
        assert gs.shape == (5, d) and row_err(gs, want[sub.cpu().long().numpy()]) <= FACTOR * ec
        assert torch.equal(gs[1], gs[2]) and not bool(gs[3].any())
        if split is None:
            assert torch.equal(gs, base[sub.long()])
    assert torch.equal(als.als_solve_rows(P['Y'], G, P['csr'], P['alpha'], P['reg'], route='fused'), base)
    assert torch.equal(als.als_solve_rows(P['Y'], G, P['csr'], P['alpha'], P['reg']), base)            # 'auto' on the device: the kernel, from one row on


@pytest.mark.parametrize('rows,n,d', SHAPES)
def test_gram_and_objective_in_double(rows, n, d):
    from arlib_amd import als
    for weighted in (False, True):
        Ph, want = reference(rows, n, d, 'b', weighted)
        P = on_device(Ph)
        val = Ph['csr'][2] if weighted else None
        G = als.gram(P['Y'])
        Gw = R.gram(Ph['Y'])
        assert G.dtype == torch.float64 and G.is_cuda and np.abs(R.f64(G) - Gw).max() <= 1e-12 * np.abs(Gw).max()
        assert torch.equal(G, G.t()) and torch.equal(G, als.gram(P['Y']))
        X = torch.from_numpy(want.copy()).float()
        Lw = R.dense_objective(X, Ph['Y'], Ph['csr'][0], Ph['csr'][1], val, P['alpha'], P['reg'])
        got = als.als_objective(X.to(DEV), P['Y'], P['csr'], P['alpha'], P['reg'], route='fused')
        assert got.dtype == torch.float64 and abs(float(got) - Lw) <= 1e-12 * Lw, (float(got), Lw)
        assert float(got) == float(als.als_objective(X.to(DEV), P['Y'], P['csr'], P['alpha'], P['reg'], G=G))          # 'auto' on the device: the kernel
        assert abs(float(als.als_objective(X.to(DEV), P['Y'], P['csr'], P['alpha'], P['reg'], route='composed')) - Lw) <= 1e-12 * Lw


def test_gram_over_more_than_one_span():
    from arlib_amd import als
    g = torch.Generator().manual_seed(5)
    for n, d in ((70_001, 16), (33_333, 128)):                          # 256 spans with a ragged last one
        Y = torch.randn(n, d, generator=g) * 0.1
        G, Gw = als.gram(Y.to(DEV)), R.gram(Y)
        assert np.abs(R.f64(G) - Gw).max() <= 1e-12 * np.abs(Gw).max()


def test_unsupported_shapes_and_indices_raise_before_any_launch(monkeypatch):
    from arlib_amd import als, _lib
    P = on_device(problem(9, 40, 24))
    G = als.gram(P['Y'])
    calls = []
    L = _lib.lib()
    for name in ('arl_als_solve_rows_f32', 'arl_als_objective_f64'):
        monkeypatch.setattr(L, name, lambda *a, _n=name: calls.append(_n) or 0)
    with pytest.raises(ValueError):
        als.als_solve_rows_kernel(P['Y'], G, P['csr'], 10.0, 0.1)       # d = 24
    with pytest.raises(ValueError):
        als.als_solve_rows(P['Y'], G, P['csr'], 10.0, 0.1, route='fused')
    Q = on_device(problem(9, 40, 32))
    G = als.gram(Q['Y'])
    bad = Q['csr'][1].clone()
    bad[3] = 40
    with pytest.raises(IndexError):
        als.als_solve_rows_kernel(Q['Y'], G, (Q['csr'][0], bad), 10.0, 0.1, check_range=True)
    with pytest.raises(IndexError):
        als.als_solve_rows_kernel(Q['Y'], G, Q['csr'], 10.0, 0.1, rows=torch.tensor([0, 9], dtype=torch.int32, device=DEV))
    with pytest.raises(IndexError):
        als.als_objective(torch.zeros(9, 32, device=DEV), Q['Y'], (Q['csr'][0], bad), 10.0, 0.1, route='fused')
    with pytest.raises(ValueError):
        als.als_solve_rows_kernel(Q['Y'], G, Q['csr'], 10.0, 0.1, split_len=0)
    with pytest.raises(Exception):
        als.als_solve_rows_kernel(Q['Y'].cpu(), G, Q['csr'], 10.0, 0.1)
    assert calls == []

"""The adjoint of the ALS row solve (csrc/arl_als.hip) on the device against the float64 restatement (tests/alsgrad_restatement.py), on the problems
of test_alsgrad_cpu.py: every case of test_als_cpu.py in both directions (as given: the full row makes every column non-empty; transposed: one
column as long as the table, which a small col_split_len cuts with a ragged last piece, and every seventh column empty), both target rules, with
split_len and col_split_len at their defaults, 8 and 5.  The upstream gradient of rows 1 and the last is scaled by 16, the empty rows' is non-zero.

Bar, in the form of test_gpu_als.py, for dY (largest row-wise relative l2 error) and for dval (largest error relative to max |dval|): the kernel's
error against float64 is at most FACTOR = 2 times that of the composed fp32 route on the same device inputs; the composed route itself is held to
the PRECONDITION bounds test_alsgrad_cpu.py derives (3 x its worst fp32 error on the CPU).  The kernels rebuild, factorise and solve A in double and
take every dot and every sum in double, which should put them below 1 x."""
import numpy as np
import pytest
import torch
import als_restatement as R0
import alsgrad_restatement as R
from test_als_cpu import SHAPES, problem, row_err, synthetic_data
from test_alsgrad_cpu import CASES, FACTOR, PRECONDITION_DY, PRECONDITION_DVAL, directed, reference, dval_err, revadv

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLITS = (None, 8, 5)


def on_device(P):
    return dict(P, Y=P['Y'].to(DEV), csr=tuple(t.to(DEV) for t in P['csr']))


def pieces(lengths, split):
    """(pieces in all, split rows or columns, whether one of them ends in a ragged piece) under the kernels' rule: longer than split -> ceil(len / split)."""
    cut = [int(l) for l in lengths if l > split]
    return sum(-(-l // split) for l in cut), len(cut), any(l % split for l in cut)


def test_the_problems_hold_what_the_cases_need():
    for rows, n, d in SHAPES:
        for transposed in (False, True):
            P = directed(rows, n, d, 'a', False, transposed)
            deg = np.diff(P['csr'][0].numpy())
            cdeg = np.bincount(P['csr'][1].numpy(), minlength=P['n'])
            if not transposed:
                assert deg[-1] == n and deg[1] == 53 and cdeg.min() >= 1 and all(deg[r] == 0 for r in range(0, rows, 7))
            else:                                                       # column rows - 1 holds every row; every seventh column is empty
                assert cdeg[-1] == n == P['rows'] and cdeg[1] == 53 and all(cdeg[c] == 0 for c in range(0, rows, 7))
                for split in (8, 5):
                    total, cut, ragged = pieces(cdeg, split)
                    assert cut >= 2 and total >= -(-n // split) + -(-53 // split)
                assert pieces(cdeg, 8)[2] and n % 8 != 0                  # the long column's last piece is ragged at 8 on every shape
    assert pieces(np.diff(problem(70, 515, 64)['csr'][0].numpy()), 5)[1] > 3


@pytest.mark.parametrize('rows,n,d,family,weighted,target,transposed', CASES)
def test_adjoint_against_float64_and_the_composed_route(rows, n, d, family, weighted, target, transposed):
    from arlib_amd import als, alsgrad
    Ph, gX, Xw, dYw, dvw = reference(rows, n, d, family, weighted, target, transposed)
    P = on_device(Ph)
    a, r, csr = P['alpha'], P['reg'], P['csr']
    G = als.gram(P['Y'])
    X = alsgrad.als_solve_rows_target(P['Y'], G, csr, a, r, target, route='fused')
    g = torch.from_numpy(gX.copy()).float().to(DEV)
    comp = alsgrad.als_adjoint_composed(P['Y'], G, csr, X, g, a, r, target)
    ecy, ecv = row_err(comp[0], dYw), dval_err(comp[1], dvw)
    assert ecy <= PRECONDITION_DY and ecv <= PRECONDITION_DVAL, (ecy, ecv)
    base = None
    for split in SPLITS:
        for csplit in SPLITS:
            got = alsgrad.als_adjoint_kernel(P['Y'], G, csr, X, g, a, r, target, split_len=split, col_split_len=csplit)
            eky, ekv = row_err(got[0], dYw), dval_err(got[1], dvw)
            print('alsgrad %s split_len %s col_split_len %s: kernel dY %.3e dval %.3e composed dY %.3e dval %.3e'
                  % ((rows, n, d, family, weighted, target, transposed), split, csplit, eky, ekv, ecy, ecv))
            assert eky <= FACTOR * ecy and ekv <= FACTOR * ecv, (split, csplit, eky, ecy, ekv, ecv)
            again = alsgrad.als_adjoint_kernel(P['Y'], G, csr, X, g, a, r, target, split_len=split, col_split_len=csplit)
            assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])          # run to run: the same bits
            if split is None and csplit is None:
                base = got
    big = max(P['rows'], P['n']) + 1                                    # split lengths that split nothing give the default's bits
    same = alsgrad.als_adjoint_kernel(P['Y'], G, csr, X, g, a, r, target, split_len=big, col_split_len=big)
    assert torch.equal(same[0], base[0]) and torch.equal(same[1], base[1])
    nod = alsgrad.als_adjoint_kernel(P['Y'], G, csr, X, g, a, r, target, want_dval=False)
    assert nod[1] is None and torch.equal(nod[0], base[0])
    fused = alsgrad.als_adjoint(P['Y'], G, csr, X, g, a, r, target, route='fused')
    assert torch.equal(fused[0], base[0]) and torch.equal(fused[1], base[1])
    auto = alsgrad.als_adjoint(P['Y'], G, csr, X, g, a, r, target)     # 'auto': the kernels only from the measured size on (None: never)
    assert torch.equal(auto[0], base[0] if alsgrad.auto_prefers_kernel(P['rows'], d) else comp[0])
    if not weighted:
        ones = alsgrad.als_adjoint_kernel(P['Y'], G, csr + (torch.ones(csr[1].numel(), device=DEV),), X, g, a, r, target)
        assert torch.equal(ones[0], base[0]) and torch.equal(ones[1], base[1])
    # the empty rows' upstream gradient is ignored
    g2 = g.clone()
    g2[(P['csr'][0][1:] == P['csr'][0][:-1])] = 1e3
    other = alsgrad.als_adjoint_kernel(P['Y'], G, csr, X, g2, a, r, target)
    assert torch.equal(other[0], base[0]) and torch.equal(other[1], base[1])


@pytest.mark.parametrize('rows,n,d', SHAPES)
def test_forward_under_the_target_rules(rows, n, d):
    from arlib_amd import als, alsgrad
    for weighted in (False, True):
        P = on_device(problem(rows, n, d, 'b', weighted))
        G = als.gram(P['Y'])
        for split in SPLITS:
            want = als.als_solve_rows_kernel(P['Y'], G, P['csr'], P['alpha'], P['reg'], split_len=split)
            got = alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], P['alpha'], P['reg'], 'stored', route='fused', split_len=split)
            assert torch.equal(got, want)
            ones = (P['csr'][0], P['csr'][1], torch.ones(P['csr'][1].numel(), device=DEV))
            rel = alsgrad.als_solve_rows_target(P['Y'], G, ones, P['alpha'], P['reg'], 'relaxed', route='fused', split_len=split)
            assert torch.equal(rel, als.als_solve_rows_kernel(P['Y'], G, ones, P['alpha'], P['reg'], split_len=split))
        if weighted:
            Xw = R.solve_rows(P['Y'], P['csr'][0], P['csr'][1], P['csr'][2], P['alpha'], P['reg'], 'relaxed')
            ec = row_err(alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], P['alpha'], P['reg'], 'relaxed', route='composed'), Xw)
            ek = row_err(alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], P['alpha'], P['reg'], 'relaxed', route='fused'), Xw)
            assert ec <= 1e-5 and ek <= FACTOR * ec, (ek, ec)            # test_gpu_als.py's bar for the solved rows
            assert torch.equal(alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], P['alpha'], P['reg'], 'relaxed'),
                               alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], P['alpha'], P['reg'], 'relaxed', route='fused'))        # 'auto': the kernel


def sweep_loss(alsgrad, multinomial_nll, allpairs, Y0, csr, route):
    rowptr, col, val = csr
    rows, n = rowptr.numel() - 1, Y0.shape[0]
    tptr, trow, tperm = allpairs.transpose_positives(rowptr, col, rows, n)
    X = alsgrad.als_solve(Y0, csr, 10.0, 0.1, 'relaxed', route, transposed=(tptr, trow, tperm))
    Y1 = alsgrad.als_solve(X, (tptr, trow, val[tperm.long()]), 10.0, 0.1, 'relaxed', route)
    return multinomial_nll(X, Y1, (rowptr, col)).sum() / rows


def test_als_solve_chained_into_a_sweep_and_a_loss():
    from arlib_amd import alsgrad, allpairs
    from arlib_amd.multinomial import multinomial_nll
    Ph = problem(40, 77, 32, 'a', True)

    def grads(dev, dt, route):
        Y0 = Ph['Y'].to(dev).to(dt).requires_grad_(True)
        val = Ph['csr'][2].to(dev).to(dt).requires_grad_(True)
        loss = sweep_loss(alsgrad, multinomial_nll, allpairs, Y0, (Ph['csr'][0].to(dev), Ph['csr'][1].to(dev), val), route)
        gy, gv = torch.autograd.grad(loss, (Y0, val))
        return float(loss), gy, gv
    lw, wy, wv = grads('cpu', torch.float64, 'composed')
    lc, cy, cv = grads(DEV, torch.float32, 'composed')
    lk, ky, kv = grads(DEV, torch.float32, 'fused')
    ecy, ecv, eky, ekv = row_err(cy, R0.f64(wy)), dval_err(cv, R0.f64(wv)), row_err(ky, R0.f64(wy)), dval_err(kv, R0.f64(wv))
    print('alsgrad sweep + nll: kernel dY0 %.3e dval %.3e composed dY0 %.3e dval %.3e' % (eky, ekv, ecy, ecv))
    assert abs(lk - lw) <= 1e-5 * abs(lw) and abs(lc - lw) <= 1e-5 * abs(lw)
    assert ecy <= PRECONDITION_DY and ecv <= PRECONDITION_DVAL
    assert eky <= FACTOR * ecy and ekv <= FACTOR * ecv
    assert torch.equal(ky, grads(DEV, torch.float32, 'fused')[1])


def test_unsupported_shapes_and_indices_raise_before_any_launch(monkeypatch):
    from arlib_amd import als, alsgrad, _lib
    P = on_device(problem(9, 40, 24))
    G = als.gram(P['Y'])
    X, g = torch.zeros(9, 24, device=DEV), torch.ones(9, 24, device=DEV)
    calls = []
    L = _lib.lib()
    for name in ('arl_als_solve_rows_target_f32', 'arl_als_adjoint_f32', 'arl_als_solve_rows_f32'):
        monkeypatch.setattr(L, name, lambda *a, _n=name: calls.append(_n) or 0)
    with pytest.raises(ValueError):
        alsgrad.als_solve_rows_target(P['Y'], G, P['csr'], 10.0, 0.1, route='fused')                    # d = 24
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(P['Y'], G, P['csr'], X, g, 10.0, 0.1, 'stored')
    with pytest.raises(ValueError):
        alsgrad.als_adjoint(P['Y'], G, P['csr'], X, g, 10.0, 0.1, 'stored', route='fused')
    with pytest.raises(ValueError):
        alsgrad.als_solve(P['Y'], P['csr'], 10.0, 0.1, route='fused')
    Q = on_device(problem(9, 40, 32))
    G = als.gram(Q['Y'])
    X, g = torch.zeros(9, 32, device=DEV), torch.ones(9, 32, device=DEV)
    bad = Q['csr'][1].clone()
    bad[3] = 40
    with pytest.raises(IndexError):
        alsgrad.als_solve_rows_target(Q['Y'], G, (Q['csr'][0], bad), 10.0, 0.1, route='fused')
    with pytest.raises(IndexError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, (Q['csr'][0], bad), X, g, 10.0, 0.1, 'relaxed')
    with pytest.raises(IndexError):
        alsgrad.als_solve(Q['Y'], (Q['csr'][0], bad), 10.0, 0.1, route='fused')
    from arlib_amd.allpairs import transpose_positives
    tptr, trow, tperm = transpose_positives(Q['csr'][0], Q['csr'][1], 9, 40)
    worse = trow.clone()
    worse[0] = 9
    with pytest.raises(IndexError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X, g, 10.0, 0.1, 'relaxed', transposed=(tptr, worse, tperm))
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X, g, 10.0, 0.1, 'relaxed', transposed=(tptr[:-1], trow, tperm))
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X, g, 10.0, 0.1, 'relaxed', col_split_len=0)
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X, g, 10.0, 0.1, 'relaxed', split_len=0)
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X[:4], g[:4], 10.0, 0.1, 'relaxed')
    with pytest.raises(ValueError):
        alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X, g, 10.0, 0.1, 'soft')
    for call in (lambda: alsgrad.als_adjoint_kernel(Q['Y'].cpu(), G, Q['csr'], X, g, 10.0, 0.1, 'relaxed'),
                 lambda: alsgrad.als_adjoint_kernel(Q['Y'], G, Q['csr'], X.cpu(), g, 10.0, 0.1, 'relaxed'),
                 lambda: alsgrad.als_solve_rows_target(Q['Y'].cpu(), G, Q['csr'], 10.0, 0.1, route='fused'),
                 lambda: alsgrad.als_solve(Q['Y'].cpu(), Q['csr'], 10.0, 0.1, route='fused')):
        with pytest.raises(Exception):
            call()
    assert calls == []


def test_revadv_on_the_fused_route():
    data = synthetic_data(60, 40, seed=5, hub=False)
    kw = dict(emb_size=16, outerEpoch=2)
    fused = revadv(data, rev_route='fused', rev_dtype='float32', rev_device=DEV, **kw)
    comp = revadv(data, rev_route='composed', rev_dtype='float32', rev_device=DEV, **kw)
    want = revadv(data, rev_route='composed', rev_dtype='float64', rev_device='cpu', **kw)
    W = want.initial_block()
    lw, gw = want.hypergradient(W)
    lc, gc = comp.hypergradient(W.float().to(DEV))
    lk, gk = fused.hypergradient(W.float().to(DEV))
    ec, ek = dval_err(gc, R0.f64(gw)), dval_err(gk, R0.f64(gw))
    print('revadv dL/dW of the first outer epoch: fused %.3e composed %.3e' % (ek, ec))
    assert abs(float(lk) - float(lw)) <= 1e-5 * abs(float(lw))
    assert ec <= PRECONDITION_DVAL and ek <= FACTOR * ec, (ek, ec)
    out = fused.posionDataAttack(None).tocsr()
    targets = sorted(set(fused.targetItem))
    fake = np.asarray(out[60:].todense())
    assert out.shape == (64, 40) and (out[:60] != fused.interact).nnz == 0
    assert np.all(fake.sum(1) == 8) and np.all(fake[:, targets] == 1) and set(np.unique(fake)) == {0.0, 1.0}
    assert len(fused.loss_log) == 2 and all(np.isfinite(fused.loss_log))

"""GPU: the row-subset hop with length-proportional pieces (spmm_rows: subset_prep_kernel, spmm_subset_pieces_kernel, subset_pieces_finish_kernel).

A listed row of len edges is cut into max(1, ceil(len / P)) pieces, P = 1024 doubled on the device until the pieces fit the caller's workspace
(n * nsplit * d floats, which also holds the piece tables).  Checked here: the float64 product at RTOL for every width class and with / without layer
tables, run-to-run bits, that a row's result depends on its own row only, the doubling, and that nothing is read from the workspace before the
prep kernel wrote it (NaN / 0xFF poison, and the tables a previous, larger call left behind)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from conftest import rel_err, RTOL
from oracle import oracle as O
from poison import poison_, compare

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U, I = 6000, 801                 # item 800 has no edge
WIDTHS = (8, 64, 128, 256)
PIECE = 1024                     # the library's starting piece length
NSPLIT = {'hub_300': 2}          # 300 x 2 pieces of 1024 edges + 2 rows do not fit 2 per row: P must double


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')
    from arlib_amd import ops
    return ops


@pytest.fixture(scope='module')
def world(ops):
    rng = np.random.default_rng(9)
    us = np.repeat(np.arange(U), 10)
    its = np.floor((I - 1) * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    val = O.norm_adj_values(rowptr, col, w)
    N = U + I
    lens = np.diff(rowptr)
    hub = int(np.argmax(lens))
    assert 1500 < lens[hub] <= 2 * PIECE and lens[N - 1] == 0
    A64 = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(N, N))
    short = rng.choice(U, 40, replace=False)
    lists = {'short': short, 'hub_once': np.concatenate([short[:20], [hub], short[20:]]), 'hub_300': np.concatenate([short[:2], np.full(300, hub)]),
             'empty_row': np.array([N - 1, 5, N - 1]), 'one': np.array([hub]),
             'prep_full': np.resize(np.concatenate([short, [hub]]), 8192), 'past_prep': np.resize(np.concatenate([short, [hub]]), 8193)}
    per_d = {}
    for d in WIDTHS:
        X = rng.standard_normal((N, d)).astype(np.float32)
        Ls = [rng.standard_normal((N, d)).astype(np.float32) for _ in range(3)]
        per_d[d] = {'X': T(X), 'L': [T(t) for t in Ls], 'AX': A64 @ X.astype(np.float64), 'Lsum': sum(t.astype(np.float64) for t in Ls)}
    return {'A': ops.CSRGraph(rowptr, col, val, DEV), 'lens': lens, 'lists': {k: v.astype(np.int32) for k, v in lists.items()}, 'hub': hub, 'd': per_d}


def expected_plan(lens, rows, nsplit, d, P=PIECE):
    n = len(rows)
    cap = (n * nsplit * d - (n + 3)) // (d + 1)
    if cap < n or n > 8192:              # no room for the piece tables / more rows than the one-workgroup prep kernel takes: equal ranges
        return None
    while True:
        s = np.maximum(1, -(-lens[rows] // P))
        if s.sum() <= cap:
            return P, int(s.sum()), np.concatenate([[0], np.cumsum(s)])
        P *= 2


@pytest.mark.parametrize('n_layers', [0, 3])
@pytest.mark.parametrize('d', WIDTHS)
def test_rows_in_pieces_match_float64_and_repeat(ops, world, d, n_layers):
    w = world['d'][d]
    layers = w['L'][:n_layers]
    for name, rows in world['lists'].items():
        n, ns = len(rows), NSPLIT.get(name, 4)
        ws = torch.zeros(n * ns * d, dtype=torch.float32, device=DEV)
        got = ops.spmm_rows(world['A'], w['X'], T(rows), layers, 0.25, nsplit=ns, workspace=ws)
        plan = ops.spmm_rows_plan(ws, n, ns, d)
        exp = expected_plan(world['lens'], rows, ns, d)
        assert (plan is None) == (exp is None), name
        if exp is not None:
            assert plan[:2] == exp[:2] and np.array_equal(plan[2].cpu().numpy(), exp[2]), name
            if name == 'hub_300':
                assert plan[0] > PIECE and plan[1] == n      # P doubled on the device
            if name == 'hub_once':
                assert plan[0] == PIECE and plan[1] > n
        ref = 0.25 * (w['AX'][rows] + (w['Lsum'][rows] if n_layers else 0.0))
        assert rel_err(got.cpu().numpy(), ref) < RTOL, name
        again = ops.spmm_rows(world['A'], w['X'], T(rows), layers, 0.25, nsplit=ns)
        assert torch.equal(got, again), name
        if name == 'empty_row' and n_layers == 0:
            assert float(got[0].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


@pytest.mark.parametrize('d', WIDTHS)
def test_a_piece_depends_on_its_own_row_only(ops, world, d):
    w = world['d'][d]
    rows = world['lists']['hub_once']
    twice = np.concatenate([rows, world['lists']['short'][::-1], [world['hub']]]).astype(np.int32)
    assert len(twice) >= 2 * len(rows)
    a = ops.spmm_rows(world['A'], w['X'], T(rows), w['L'], 0.25, nsplit=16)
    b = ops.spmm_rows(world['A'], w['X'], T(twice), w['L'], 0.25, nsplit=16)
    assert torch.equal(a, b[:len(rows)])
    assert torch.equal(b[len(rows) - 1 - 20], b[-1])                     # the hub row, listed twice


@pytest.mark.parametrize('d', WIDTHS)
def test_rows_workspace_is_written_before_it_is_read(ops, world, d):
    w = world['d'][d]
    for name in ('hub_once', 'hub_300', 'empty_row', 'one'):
        rows = T(world['lists'][name])
        n, ns = rows.numel(), NSPLIT.get(name, 4)
        clean = ops.spmm_rows(world['A'], w['X'], rows, w['L'], 0.25, nsplit=ns, workspace=torch.zeros(n * ns * d, dtype=torch.float32, device=DEV))
        nan_ws = poison_(torch.empty(n * ns * d, dtype=torch.float32, device=DEV))
        ff_ws = poison_(torch.empty(4 * n * ns * d, dtype=torch.uint8, device=DEV)).view(torch.float32)
        for ws in (nan_ws, ff_ws):
            got = ops.spmm_rows(world['A'], w['X'], rows, w['L'], 0.25, nsplit=ns, workspace=ws)
            assert compare(clean, got) == [], name
    # a stale, larger piece count (and its offsets and piece -> row map) left by the previous call on the same workspace
    big, small = world['lists']['hub_300'], np.resize(world['lists']['short'], len(world['lists']['hub_300'])).astype(np.int32)
    n, ns = len(big), 4
    ws = torch.zeros(n * ns * d, dtype=torch.float32, device=DEV)
    ops.spmm_rows(world['A'], w['X'], T(big), w['L'], 0.25, nsplit=ns, workspace=ws)
    stale = ops.spmm_rows_plan(ws, n, ns, d)
    got = ops.spmm_rows(world['A'], w['X'], T(small), w['L'], 0.25, nsplit=ns, workspace=ws)
    now = ops.spmm_rows_plan(ws, n, ns, d)
    assert stale[1] > now[1] == n and now[0] == PIECE
    clean = ops.spmm_rows(world['A'], w['X'], T(small), w['L'], 0.25, nsplit=ns, workspace=torch.zeros(n * ns * d, dtype=torch.float32, device=DEV))
    assert compare(clean, got) == []

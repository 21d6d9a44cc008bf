"""GPU: a hop over a WHOLE blocked plan in one native call (arl_spmm_blocked_*_sets_f32) against one call per row set.

The whole-plan call launches the sets and then ONE combine for the split rows of all of them; its masked form runs the sets in ONE grid where
they agree on rows_per_wave.  Every wave runs the records it runs in the per-set calls, in the same order, and a split row adds the same pieces
in the same order, so every case here asks for torch.equal, on outputs pre-filled with a sentinel (a row neither path writes stays equal, a row
only one of them writes does not).  Small forced plans: 470 user rows and 90 item rows, a split threshold of 16 edges so that BOTH sets have
split rows, wave counts that are no multiple of the waves per workgroup, and item rows heavy enough (> 4096 edges per 32 rows) that the plan
gives them one wave per workgroup next to the user rows' four (the merged grid then runs both with one) and longer record streams per wave
than the user rows have (the merged grid then starts with the SECOND set)."""
import ctypes as C
import numpy as np
import pytest
import torch
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U, I = 470, 90
N = U + I
SENTINEL = 12345.0
PLANS = {
    'split': dict(hub=16, piece=16),                                   # both sets split; waves per workgroup 4 (users) and 1 (items)
    'wpg4': dict(hub=16, piece=14, wpg=4),                             # one workgroup shape for both sets, 37 and 31 waves
    'wpg2': dict(hub=16, piece=16, wpg=2, unroll=16),
    'rpw16': dict(hub=16, piece=16, rows_per_wave=16, unroll=16),
    'items_split': dict(hub=64, piece=32),                             # no user row is longer than 64 edges: one set without split rows
    'one_set': dict(hub=16, piece=16, split=None),                     # a plan with one set only
}


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')
    from arlib_amd import ops
    return ops


@pytest.fixture(scope='module')
def csr():
    rng = np.random.default_rng(5)
    deg = rng.integers(24, 48, U)
    us = np.repeat(np.arange(U), deg)
    its = np.floor(I * rng.random(len(us)) ** 1.5).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    return rowptr, col, O.norm_adj_values(rowptr, col, w), us, its


@pytest.fixture(scope='module')
def planned(ops, csr):
    out = {}
    for name, kw in PLANS.items():
        kw = dict(kw)
        A = ops.CSRGraph(*csr[:3], DEV)
        A.enable_blocked(split=kw.pop('split', U), **kw)
        assert A.blocked.hub is None and A.blocked.n_hub == 0             # every row is in the plan: the whole-plan route
        out[name] = A
    sets = {k: [(s['n_waves'], s['wpg'], s['n_split']) for s in A.blocked.sets] for k, A in out.items()}
    assert all(ns > 0 for _, _, ns in sets['split']) and [w for _, w, _ in sets['split']] == [4, 1], sets
    st = out['split'].blocked.sets
    assert st[1]['rec_col'].numel() // st[1]['n_waves'] > st[0]['rec_col'].numel() // st[0]['n_waves']     # merged grid order != array order
    for k in ('split', 'wpg4', 'wpg2'):
        assert any(nw % w for nw, w, _ in sets[k]), sets                 # a last workgroup with surplus waves
    assert all(nw % w for nw, w, _ in sets['wpg4']), sets                 # ... in either set
    assert [ns > 0 for _, _, ns in sets['items_split']] == [False, True], sets
    assert len(sets['one_set']) == 1 and sets['one_set'][0][2] > 0, sets
    return out


class Route:
    """Runs a callable on the whole-plan route and on the per-set route and says which native entries each took."""

    def __init__(self, ops, monkeypatch):
        self.ops, self.mp, self.calls = ops, monkeypatch, []
        L = ops._lib.lib()
        for nm in ops._lib.EXPORTS:
            if nm.startswith('arl_spmm_blocked'):
                monkeypatch.setattr(L, nm, (lambda f, n: lambda *a: (self.calls.append(n), f(*a))[1])(getattr(L, nm), nm), raising=False)

    def both(self, fn, n_sets, entry):
        del self.calls[:]
        self.mp.setattr(self.ops, 'HOP_SETS', True)
        whole = fn()
        assert self.calls == [entry.replace('_f32', '_sets_f32')], self.calls
        del self.calls[:]
        self.mp.setattr(self.ops, 'HOP_SETS', False)
        per_set = fn()
        assert self.calls == [entry] * n_sets, self.calls
        self.mp.setattr(self.ops, 'HOP_SETS', True)
        return whole, per_set


@pytest.fixture
def route(ops, monkeypatch):
    return Route(ops, monkeypatch)


def bitmap(ops, nodes):
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    if len(nodes):
        ops.mark_bits_(bits, T(np.asarray(nodes, np.int32)), True, N)
    return bits


def operands(d, nodes, seed):
    rng = np.random.default_rng(seed)
    X = np.zeros((N, d), np.float32)
    X[nodes] = rng.standard_normal((len(nodes), d)).astype(np.float32)
    zf = (rng.random(N) < 0.3).astype(np.uint8)
    Z = rng.standard_normal((N, d)).astype(np.float32) * zf[:, None]
    return T(X), T(Z), T(zf)


def sentinel(d):
    return torch.full((N, d), SENTINEL, device=DEV)


MASKS = {'clear': lambda rng: np.zeros(0, np.int64), 'all': lambda rng: np.arange(N),
         'sparse': lambda rng: np.unique(np.concatenate([rng.choice(U, 40, replace=False), U + rng.choice(I, 25, replace=False), [N - 1]]))}


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('plan', list(PLANS))
def test_masked_whole_plan_equals_per_set_and_unmasked(ops, planned, route, plan, d):
    A = planned[plan]
    n_sets = len(A.blocked.sets)
    for k, (name, pick) in enumerate(MASKS.items()):
        nodes = pick(np.random.default_rng(k))
        X, Z, zf = operands(d, nodes, 10 * k + d)
        bits = bitmap(ops, nodes)
        for with_z in (True, False):
            args = (0.5, 0.25, Z, zf) if with_z else (0.5, 0.0, None, None)
            whole, per_set = route.both(lambda: ops.spmm_flagged(A, X, bits, *args, out=sentinel(d)), n_sets, 'arl_spmm_blocked_flagged_f32')
            assert torch.equal(whole, per_set), (plan, name, with_z)
            assert not bool((whole == SENTINEL).any()), (plan, name, with_z)                     # every row of the table is written
            dense, dense_ps = route.both(lambda: ops.spmm_flagged(A, X, None, *args, out=sentinel(d)), n_sets, 'arl_spmm_blocked_f32')
            assert torch.equal(dense, dense_ps), (plan, name, with_z)
            assert torch.equal(whole, dense), (plan, name, with_z)                               # masked whole-plan = unmasked whole-plan, same operand
        if name != 'clear':
            assert float(whole.abs().max()) > 0


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('plan', ['split', 'rpw16', 'items_split', 'one_set'])
def test_every_epilogue_through_the_single_combine(ops, planned, route, plan, d):
    A = planned[plan]
    n_sets = len(A.blocked.sets)
    rng = np.random.default_rng(d + len(plan))
    X = T(rng.standard_normal((N, d)).astype(np.float32))
    _, Z, zf = operands(d, np.arange(N), 3)
    rs = T(rng.random(N).astype(np.float32) + 0.5)
    # plain, with a row scale
    a, b = route.both(lambda: ops.spmm(A, X, 0.5, 0.25, Z, out=sentinel(d)), n_sets, 'arl_spmm_blocked_f32')
    assert torch.equal(a, b) and not bool((a == SENTINEL).any())
    a, b = route.both(lambda: ops.spmm(A, X, 0.5, 0.0, None, out=sentinel(d), row_scale=rs), n_sets, 'arl_spmm_blocked_rscale_f32')
    assert torch.equal(a, b) and not bool((a == SENTINEL).any())
    # layer sum, out of place (with the product stored) and in place
    S_in = T(rng.standard_normal((N, d)).astype(np.float32))

    def layersum(in_place):
        S = S_in.clone() if in_place else sentinel(d)
        Y = None if in_place else sentinel(d)
        ops.spmm_layersum(A, X, S if in_place else S_in, S, Y)
        return S if in_place else torch.cat([S, Y])
    for in_place in (False, True):
        a, b = route.both(lambda: layersum(in_place), n_sets, 'arl_spmm_blocked_layersum_f32')
        assert torch.equal(a, b) and not bool((a == SENTINEL).any()), in_place
    # Adam, two steps on the same state
    P0, M0, V0 = (T(rng.standard_normal((N, d)).astype(np.float32)), T(rng.standard_normal((N, d)).astype(np.float32) * 0.1),
                  T(rng.random((N, d)).astype(np.float32) * 0.01))

    def adam():
        P, M, V = P0.clone(), M0.clone(), V0.clone()
        for step in (1, 2):
            ops.spmm_adam(A, X, 0.5, 0.25, Z, P, M, V, 0.01, step, zflags=zf)
        return torch.cat([P, M, V])
    del route.calls[:]
    route.mp.setattr(ops, 'HOP_SETS', True)
    a = adam()
    assert route.calls == ['arl_spmm_blocked_adam_sets_f32'] * 2
    route.mp.setattr(ops, 'HOP_SETS', False)
    b = adam()
    route.mp.setattr(ops, 'HOP_SETS', True)
    assert torch.equal(a, b) and not torch.equal(a, torch.cat([P0, M0, V0]))


@pytest.mark.parametrize('d', [64, 128])
def test_rows_from_skips_the_first_set(ops, planned, route, d):
    A = planned['split']
    X = T(np.random.default_rng(1).standard_normal((N, d)).astype(np.float32))
    a, b = route.both(lambda: ops.spmm(A, X, out=sentinel(d), rows_from=U), 1, 'arl_spmm_blocked_f32')
    full = ops.spmm(A, X)
    assert torch.equal(a, b) and torch.equal(a[U:], full[U:])
    assert bool((a[:U] == SENTINEL).all())                                                      # neither the first set's launch nor its split rows' combine ran


@pytest.mark.parametrize('d', [64, 128])
def test_sets_with_different_rows_per_wave_fall_back(ops, planned, d):
    """The user rows of the 32-row plan and the item rows of the 16-row plan as ONE array of sets, their split tables and piece areas joined by
    hand the way the plan joins its own: the masked whole-plan call cannot merge them and must launch them one by one."""
    L = ops._lib.lib()
    b32, b16 = planned['split'].blocked, planned['rpw16'].blocked
    s0, s1 = b32.struct(0, d), b16.struct(1, d)
    st0, st1 = b32.sets[0], b16.sets[1]
    assert s0.rows_per_wave == 32 and s1.rows_per_wave == 16 and st0['n_split'] > 0 and st1['n_split'] > 0
    partial = torch.empty((st0['n_pieces'] + st1['n_pieces']) * 64, device=DEV)
    s0.partial = partial.data_ptr()
    s1.partial = partial.data_ptr() + st0['n_pieces'] * 64 * 4
    rows = torch.cat([st0['split_row'], st1['split_row']]).contiguous()
    first = torch.cat([st0['split_first'], st1['split_first'] + st0['n_pieces']]).contiguous()
    count = torch.cat([st0['split_count'], st1['split_count']]).contiguous()
    arr = (ops._lib.arl_blocked * 2)(s0, s1)
    hop = ops._lib.arl_blocked_hop(rows.numel(), rows.data_ptr(), first.data_ptr(), count.data_ptr(), partial.data_ptr(), None)
    nodes = MASKS['sparse'](np.random.default_rng(2))
    X, Z, zf = operands(d, nodes, 77)
    bits = bitmap(ops, nodes)
    whole, per_set = sentinel(d), sentinel(d)
    args = (0.5, 0.25, Z.data_ptr(), zf.data_ptr())
    assert L.arl_spmm_blocked_flagged_sets_f32(arr, 2, 0, C.byref(hop), X.data_ptr(), d, bits.data_ptr(), *args, whole.data_ptr(), None) == 0
    for s in (s0, s1):
        assert L.arl_spmm_blocked_flagged_f32(C.byref(s), X.data_ptr(), d, bits.data_ptr(), *args, per_set.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(whole, per_set) and not bool((whole == SENTINEL).any())
    # what the whole-plan entries refuse: a first set past the array, split rows without their joined tables
    assert L.arl_spmm_blocked_flagged_sets_f32(arr, 2, 3, C.byref(hop), X.data_ptr(), d, bits.data_ptr(), *args, whole.data_ptr(), None) == -3
    assert L.arl_spmm_blocked_flagged_sets_f32(arr, 2, 0, None, X.data_ptr(), d, bits.data_ptr(), *args, whole.data_ptr(), None) == -1
    assert L.arl_spmm_blocked_flagged_sets_f32(arr, 2, 0, C.byref(hop), X.data_ptr(), d, None, *args, whole.data_ptr(), None) == -1
    assert L.arl_spmm_blocked_sets_f32(arr, 2, 0, C.byref(hop), X.data_ptr(), 32, *args, whole.data_ptr(), None) == -2


def test_three_steps_equal_the_per_set_route(ops, csr, monkeypatch):
    """PropagationEngine.step on schedule='blocked' over a plan with split rows in both sets: three steps through the whole-plan calls leave the bits
    of the same three steps with _spmm_dispatch on the per-set route."""
    from arlib_amd import engine
    rng = np.random.default_rng(21)
    d, L, B = 64, 3, 256
    us, its = csr[3], csr[4]
    E0 = ((rng.random((N, d)) * 2 - 1) * 0.05).astype(np.float32)
    batches = []
    for _ in range(3):
        sel = rng.integers(0, len(us), B)
        batches.append((T(us[sel].copy()), T(its[sel].copy()), T(rng.integers(0, I, B).astype(np.int32))))
    out = {}
    for whole in (True, False):
        monkeypatch.setattr(ops, 'HOP_SETS', whole)
        A = ops.CSRGraph(*csr[:3], DEV).enable_blocked(split=U, hub=16, piece=16)
        eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, DEV, table=T(E0), schedule='blocked')
        assert eng.A.blocked is not None and eng.A.blocked.hub is None and all(s['n_split'] > 0 for s in eng.A.blocked.sets)
        losses = [eng.step(*b).clone() for b in batches]
        out[whole] = (torch.stack(losses), eng.E0.clone(), eng.m.clone(), eng.v.clone())
    for a, b in zip(out[True], out[False]):
        assert torch.equal(a, b)
    assert not torch.equal(out[True][1], T(E0))

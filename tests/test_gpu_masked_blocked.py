"""GPU: the flag-masked hop on the register-blocked plan (arl_spmm_blocked_flagged_f32).

A record the mask skips would have added fmaf(v, 0, acc) = acc, so on an operand that is zero outside the flagged rows the masked hop must have the
BITS of the unmasked hop on the same plan (ops.spmm), for every flag set.  That holds for every row the plan itself produces, split rows included.
Rows the plan leaves to the chunked CSR kernel (its hub rows: only with split_hubs=False or a row set below min_waves) go through
arl_spmm_csr_flagged_f32 in the masked hop and arl_spmm_csr_f32 in the unmasked one, which add a row's edges in different orders; those rows are held to
the float64 product at RTOL, like every CSR kernel, and bitwise to arl_spmm_csr_flagged_f32 on the hub graph alone, the code that produces them."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
from conftest import rel_err, RTOL
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U, I = 6000, 800                 # N = 6800 is no multiple of 32: the last node's bit lies in a partial bitmap word, and it has edges


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')
    from arlib_amd import ops, engine
    return ops, engine


@pytest.fixture(scope='module')
def graph():
    rng = np.random.default_rng(9)
    us = np.repeat(np.arange(U), 10)
    its = np.floor(I * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    val = O.norm_adj_values(rowptr, col, w)
    assert np.diff(rowptr).max() > 1500
    N = U + I
    assert N % 32 != 0 and rowptr[N] - rowptr[N - 1] > 0                 # the 'last' flag set is gathered by real records
    A64 = sp.csr_matrix((val.astype(np.float64), col, rowptr), shape=(U + I, U + I))
    return {'csr': (rowptr, col, val), 'A64': A64, 'us': us, 'its': its, 'hub': int(np.argmax(np.diff(rowptr)))}


PLANS = {'split': dict(hub=256, piece=256, split_hubs=True), 'hub': dict(hub=256, split_hubs=False), 'rpw16': dict(hub=512, rows_per_wave=16, unroll=16)}


@pytest.fixture(scope='module')
def planned(mods, graph):
    ops, _ = mods
    out = {}
    for name, kw in PLANS.items():
        A = ops.CSRGraph(*graph['csr'], DEV)
        A.enable_blocked(split=U, **kw)
        out[name] = A
    assert sum(s['n_split'] for s in out['split'].blocked.sets) > 0 and out['split'].blocked.n_hub == 0
    assert out['hub'].blocked.n_hub > 0
    return out


def flag_sets(graph, A):
    N = U + I
    rng = np.random.default_rng(3)
    st = A.blocked.sets[0]
    pad_cols = (st['rec_col'][st['pad_pos']].cpu().numpy() & 0xffffff)
    assert pad_cols.size > 0
    batch = np.concatenate([rng.choice(U, 512, replace=False), U + rng.integers(0, I, 1024), [graph['hub']]])
    batch = np.unique(batch)
    return {'empty': np.zeros(0, np.int64), 'all': np.arange(N), 'one': np.array([1234]), 'last': np.array([N - 1]), 'batch': batch,
            'padded': np.unique(pad_cols)[:40]}


def run_case(ops, graph, A, d, nodes, seed=0):
    N = U + I
    rng = np.random.default_rng(100 + seed)
    X = np.zeros((N, d), np.float32)
    X[nodes] = rng.standard_normal((len(nodes), d)).astype(np.float32)
    zf = (rng.random(N) < 0.3).astype(np.uint8)
    Z = rng.standard_normal((N, d)).astype(np.float32) * zf[:, None]
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    if len(nodes):
        ops.mark_bits_(bits, T(nodes.astype(np.int32)), True, N)
    Xd, Zd, zfd = T(X), T(Z), T(zf)
    got = ops.spmm_flagged(A, Xd, bits, 0.5, 0.25, Zd, zfd)
    again = ops.spmm_flagged(A, Xd, bits, 0.5, 0.25, Zd, zfd)
    dense = ops.spmm(A, Xd, 0.5, 0.25, Zd)
    AX = graph['A64'] @ X.astype(np.float64)
    ref = 0.5 * AX + 0.25 * Z.astype(np.float64)
    hub_only = None
    if A.blocked.hub is not None:            # the hub rows alone, through the CSR flagged kernel (other rows of the buffer stay zero)
        assert getattr(A.blocked.hub, 'blocked', None) is None
        hub_only = ops.spmm_flagged(A.blocked.hub, Xd, bits, 0.5, 0.25, Zd, zfd, out=torch.zeros(N, d, device=DEV))
    return got, again, dense, ref, AX, hub_only


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('plan', list(PLANS))
def test_masked_blocked_has_the_bits_of_the_unmasked_hop(mods, graph, planned, plan, d):
    ops, _ = mods
    A = planned[plan]
    hub_rows = A.blocked._hub_rows.cpu().numpy()
    keep = np.ones(U + I, bool); keep[hub_rows] = False
    keep_d = T(keep)
    for k, (name, nodes) in enumerate(flag_sets(graph, A).items()):
        got, again, dense, ref, AX, hub_only = run_case(ops, graph, A, d, nodes, k)
        assert torch.equal(got, again), (name, 'two calls differ')
        if len(hub_rows) == 0:
            assert torch.equal(got, dense), name
        else:
            assert torch.equal(got[keep_d], dense[keep_d]), name
        assert not torch.isnan(got).any()
        assert rel_err(got.cpu().numpy(), ref) < RTOL, name
        if len(hub_rows):
            assert rel_err(got.cpu().numpy()[hub_rows], ref[hub_rows]) < RTOL, name
            assert torch.equal(got[T(hub_rows)], hub_only[T(hub_rows)]), name
            if name in ('all', 'batch'):
                assert (np.abs(AX[hub_rows]).max(1) > 0).all() and bool((got[T(hub_rows)].abs().amax(1) > 0).all()), name
        if name == 'last':                       # the last node's neighbours, and only they, receive a product: a missed hit at the bitmap's tail shows here
            rowptr, col, _ = graph['csr']
            nb = col[rowptr[U + I - 1]:rowptr[U + I]]
            prod = (got - T(ref - 0.5 * AX).float()).abs().amax(1).cpu().numpy()        # what the hop added to beta * Z
            assert len(nb) > 0 and (np.abs(AX[nb]).max(1) > 0).all() and (prod[nb] > 0).all(), name
            others = np.ones(U + I, bool); others[nb] = False
            assert float(np.abs(AX[others]).max()) == 0.0


def test_masked_hop_takes_the_blocked_route(mods, graph, planned, monkeypatch):
    ops, _ = mods
    L = ops._lib.lib()
    calls = []
    for nm in ('arl_spmm_blocked_flagged_f32', 'arl_spmm_csr_flagged_f32'):
        fn = getattr(L, nm)
        monkeypatch.setattr(L, nm, (lambda f, n: lambda *a: (calls.append(n), f(*a))[1])(fn, nm), raising=False)
    N = U + I
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    X = torch.zeros(N, 64, device=DEV)
    ops.spmm_flagged(planned['hub'], X, bits)
    assert calls == ['arl_spmm_blocked_flagged_f32'] * len(planned['hub'].blocked.sets) + ['arl_spmm_csr_flagged_f32']
    del calls[:]
    ops.spmm_flagged(ops.CSRGraph(*graph['csr'], DEV), X, bits)
    assert calls == ['arl_spmm_csr_flagged_f32']
    del calls[:]
    ops.spmm_flagged(planned['split'], torch.zeros(N, 32, device=DEV), bits)          # no plan for this width
    assert calls == ['arl_spmm_csr_flagged_f32']


@pytest.mark.parametrize('L', [2, 3])
def test_blocked_sparse_step_equals_dense_step(mods, graph, L):
    """One engine on schedule='blocked' (masked hop on the plan, row-subset hop in pieces) against step_dense on 'csr'."""
    ops, engine = mods
    rng = np.random.default_rng(9 + L)
    d, B = 64, 512
    us, its = graph['us'], graph['its']
    E0 = ((rng.random((U + I, d)) * 2 - 1) * 0.05).astype(np.float32)
    ea = engine.PropagationEngine(ops.CSRGraph(*graph['csr'], DEV), U, I, d, L, 1e-4, 0.005, DEV, table=T(E0), schedule='blocked')
    eb = engine.PropagationEngine(ops.CSRGraph(*graph['csr'], DEV), U, I, d, L, 1e-4, 0.005, DEV, table=T(E0), schedule='csr')
    assert ea.A.blocked is not None and eb.A.blocked is None
    sel = rng.integers(0, len(us), B)
    bu, bp, bn = T(us[sel].copy()), T(its[sel].copy()), T(rng.integers(0, I, B).astype(np.int32))
    bu[:50] = bu[0]; bp[:80] = bp[1]; bn[:30] = bp[1]                    # heavy duplicates, item both positive and negative
    la = ea.step(bu, bp, bn).cpu().numpy()
    lb = eb.step_dense(bu, bp, bn).cpu().numpy()
    assert np.allclose(la, lb, rtol=RTOL, atol=0)
    assert rel_err(ea.E0.cpu().numpy(), eb.E0.cpu().numpy()) < RTOL
    assert rel_err(ea.m.cpu().numpy(), eb.m.cpu().numpy()) < RTOL and rel_err(ea.v.cpu().numpy(), eb.v.cpu().numpy()) < RTOL
    assert float(ea.G.abs().max()) == 0.0 and int(ea.flags.max()) == 0 and int(ea.bits.abs().max()) == 0 and int(ea.dup_bits.abs().max()) == 0

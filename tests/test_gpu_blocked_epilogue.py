"""The register-blocked hop's epilogue (spmm_blocked64_kernel): row ids, flags and row scales are read once per wave and the output rows
are loaded and stored in groups.  Small plans forced through CSRGraph.enable_blocked, at the shapes where the grouped form can go wrong:
waves with padding slots (row counts that are no multiple of rows_per_wave, a set smaller than one wave), waves without any (whole
groups only), pieces of split rows between ordinary rows, flags mixed inside a wave, with and without a row scale, d = 64 and both
halves of d = 128, the masked build, 16 and 32 loads in flight.

Exact checks: with power-of-two alpha / beta the products alpha * a and beta * z are exact, so the fused epilogue and torch's unfused
fp32 expression round once, alike; the layer sum is one fp32 add; the masked build adds the same products in the same order.  The
Adam epilogue is held to the suite's bar (RTOL) against spmm_flagged + adam_dense, as the existing tests hold it against the oracle pair,
and every mode to RTOL against a float64 restatement."""
import copy
import numpy as np
import pytest
import torch
from conftest import rel_err, RTOL

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
SENTINEL = 12345.0
GRAPHS = [(70, 45), (64, 13)]                       # (users, items): ragged sets | whole user waves and an item set smaller than one wave
PLANS = [(16, 16), (32, 16), (32, 32)]              # (rows_per_wave, unroll)
HUB, PIECE = 16, 8                                  # rows above 16 edges are dealt as pieces of <= 8 edges
_CACHE = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on the MI355X box)')
    from arlib_amd import ops as _ops
    return _ops


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def graph(ops, U, I, rpw, unroll):
    """Symmetric bipartite adjacency: 2-6 items per user (1-2 on the 13-item graph, so that most of its item rows stay below the hub
    threshold), items 0 and 1 rated by every user, user 3 rating every item (split rows in both sets of the 70 x 45 graph), user 5
    isolated (an empty row)."""
    key = (U, I, rpw, unroll)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * U + I)
        pairs = set()
        for u in range(U):
            for it in rng.choice(I, size=int(rng.integers(2, 7) if I > 16 else rng.integers(1, 3)), replace=False):
                pairs.add((u, int(it)))
            pairs.add((u, 0)); pairs.add((u, 1))
        for it in range(I):
            pairs.add((3, it))
        pairs = sorted(p for p in pairs if p[0] != 5)
        N = U + I
        Md = np.zeros((N, N), np.float64)
        for u, it in pairs:
            Md[u, U + it] = 1.0; Md[U + it, u] = 1.0
        rowptr = np.concatenate([[0], np.cumsum((Md != 0).sum(1))]).astype(np.int64)
        col = np.nonzero(Md)[1].astype(np.int32)
        val = (0.1 + 0.9 * rng.random(len(col))).astype(np.float32)
        Md[np.nonzero(Md)] = val.astype(np.float64)
        A = ops.CSRGraph(rowptr, col, val, DEV).enable_blocked(split=U, rows_per_wave=rpw, hub=HUB, piece=PIECE, unroll=unroll)
        bp = A.blocked
        assert bp is not None and len(bp.sets) == 2 and bp.hub is None
        wr = [st['wave_rows'].cpu().numpy() for st in bp.sets]
        k = 8 if unroll == 32 else 4                                       # the largest group the kernel uses
        assert any((w == -1).any() for w in wr)                            # a padded wave
        gw = [w.reshape(len(w), -1, k) for w in wr]
        whole = [np.logical_and.accumulate((q != -1).all(2), axis=1) & (w >= 0).any(1)[:, None] for q, w in zip(gw, wr)]     # groups before a wave's first padding slot
        assert any(h.any() for h in whole)
        assert any((h & (q < -1).any(2)).any() for h, q in zip(whole, gw))                     # one of them with a piece in it
        assert any(((w >= 0) & (np.roll(w, 1, 1) < -1))[:, 1:].any() for w in wr)              # pieces beside ordinary rows
        if (U, I) == (64, 13):
            assert (wr[0] >= 0).all() and I < rpw                          # whole user waves, nothing else; an item set below one wave
        _CACHE[key] = dict(A=A, M=Md, U=U, I=I, N=N, wr=wr, split=[st['split_row'].cpu().numpy() for st in bp.sets])
    return _CACHE[key]


def flags(g, pattern):
    zf = np.zeros(g['N'], np.uint8)
    if pattern == 'set':
        zf[:] = 1
    elif pattern == 'alternating':                                         # odd slots of every wave, every other split row
        for w, sp in zip(g['wr'], g['split']):
            odd = w[:, 1::2]
            zf[odd[odd >= 0]] = 1
            zf[sp[::2]] = 1
    elif pattern == 'last':                                                # the last ordinary row of every wave only
        for w in g['wr']:
            for row in w:
                if (row >= 0).any():
                    zf[row[np.nonzero(row >= 0)[0][-1]]] = 1
    else:
        assert pattern == 'clear'
    return zf


def inputs(g, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((g['N'], d)).astype(np.float32)
    Z = rng.standard_normal((g['N'], d)).astype(np.float32)
    return X, Z


def poisoned(Z, zf):
    """Z with NaN on the rows whose flag is clear: the epilogue must not let them into the result."""
    Zn = Z.copy()
    Zn[zf == 0] = np.nan
    return Zn


CASES = [(U, I, rpw, unr, d) for (U, I) in GRAPHS for (rpw, unr) in PLANS for d in (64, 128)]
case = pytest.mark.parametrize('U,I,rpw,unroll,d', CASES)


@case
def test_axpby_flags_and_row_scale_exact(ops, U, I, rpw, unroll, d):
    g = graph(ops, U, I, rpw, unroll)
    A = g['A']
    X, Z = inputs(g, d, 7 + d)
    a = ops.spmm(A, T(X))                                                  # identity epilogue: the raw row sums of this plan
    assert rel_err(a.cpu().numpy(), g['M'] @ X.astype(np.float64)) < RTOL
    rs = T((0.5 + np.random.default_rng(3).random(g['N'])).astype(np.float32))
    for alpha, beta in ((1.0, 1.0), (0.25, 1.0), (0.5, 0.25)):
        assert torch.equal(ops.spmm(A, T(X), alpha), alpha * a)
        assert torch.equal(ops.spmm(A, T(X), alpha, beta, T(Z)), alpha * a + beta * T(Z))              # Z without flags: every row reads it
        assert torch.equal(ops.spmm(A, T(X), alpha, row_scale=rs), (alpha * rs)[:, None] * a)
        assert torch.equal(ops.spmm(A, T(X), alpha, beta, T(Z), row_scale=rs), (alpha * rs)[:, None] * a + beta * T(Z))
        for pattern in ('clear', 'set', 'alternating', 'last'):
            zf = flags(g, pattern)
            want = torch.where(T(zf)[:, None] != 0, alpha * a + beta * T(Z), alpha * a)
            got = ops.spmm_flagged(A, T(X), None, alpha, beta, T(poisoned(Z, zf)), T(zf))
            assert torch.equal(got, want), pattern
            ref = alpha * (g['M'] @ X.astype(np.float64)) + beta * Z.astype(np.float64) * zf[:, None]
            assert rel_err(got.cpu().numpy(), ref) < RTOL


@case
def test_layersum_exact(ops, U, I, rpw, unroll, d):
    g = graph(ops, U, I, rpw, unroll)
    A = g['A']
    X, Z = inputs(g, d, 11 + d)
    a = ops.spmm(A, T(X))
    S_in = T(Z); S = torch.full_like(S_in, SENTINEL); Y = torch.full_like(S_in, SENTINEL)
    ops.spmm_layersum(A, T(X), S_in, S, Y)
    assert torch.equal(Y, a) and torch.equal(S, S_in + a)
    S2 = T(Z)
    ops.spmm_layersum(A, T(X), S2, S2)                                     # in place, no Y
    assert torch.equal(S2, S_in + a)
    assert rel_err(S2.cpu().numpy(), Z.astype(np.float64) + g['M'] @ X.astype(np.float64)) < RTOL


@case
def test_masked_build_equals_unmasked(ops, U, I, rpw, unroll, d):
    g = graph(ops, U, I, rpw, unroll)
    A, N = g['A'], g['N']
    X, Z = inputs(g, d, 13 + d)
    zf = flags(g, 'alternating')
    rng = np.random.default_rng(17)
    for name, keep in (('empty', np.zeros(N, bool)), ('full', np.ones(N, bool)), ('sparse', rng.random(N) < 0.15)):
        words = np.zeros((N + 31) // 32, np.uint32)
        np.bitwise_or.at(words, np.nonzero(keep)[0] >> 5, (np.uint32(1) << (np.nonzero(keep)[0] & 31).astype(np.uint32)))
        Xm = X * keep[:, None]
        bits = T(words.view(np.int32))
        for alpha, beta in ((1.0, 1.0), (0.5, 0.25)):
            got = ops.spmm_flagged(A, T(Xm), bits, alpha, beta, T(poisoned(Z, zf)), T(zf))
            assert torch.equal(got, ops.spmm_flagged(A, T(Xm), None, alpha, beta, T(poisoned(Z, zf)), T(zf))), name
            assert torch.equal(ops.spmm_flagged(A, T(Xm), bits, alpha), ops.spmm(A, T(Xm), alpha)), name
            ref = alpha * (g['M'] @ Xm.astype(np.float64)) + beta * Z.astype(np.float64) * zf[:, None]
            assert rel_err(got.cpu().numpy(), ref) < RTOL


def adam64(p, g, m, v, lr, t, b1=0.9, b2=0.999, eps=1e-8):
    m = m + (g - m) * (1 - b1)
    v = v * b2 + (1 - b2) * g * g
    p = p - lr / (1 - b1 ** t) * (m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps))
    return p, m, v


@case
def test_adam_epilogue_two_steps(ops, U, I, rpw, unroll, d):
    """Fused Adam epilogue against spmm_flagged + adam_dense on the same tables, and against float64; the second step reads the moments
    the first one wrote.  (Moments well away from zero: with v ~ eps^2 Adam's update turns rounding differences of g into whole steps.)"""
    g = graph(ops, U, I, rpw, unroll)
    A, N = g['A'], g['N']
    rng = np.random.default_rng(19 + d)
    P = rng.standard_normal((N, d)).astype(np.float32) * 0.1
    M = rng.standard_normal((N, d)).astype(np.float32) * 0.01
    V = rng.random((N, d)).astype(np.float32) * 1e-4 + 1e-6
    for pattern in ('alternating', None):
        zf = flags(g, pattern) if pattern else None
        fused, pair = [T(P), T(M), T(V)], [T(P), T(M), T(V)]
        r64 = [P.astype(np.float64), M.astype(np.float64), V.astype(np.float64)]
        for t in (7, 8):
            X, Z = inputs(g, d, 23 + d + t)
            Zp = poisoned(Z, zf) if pattern else Z
            ops.spmm_adam(A, T(X), 0.25, 1.0, T(Zp), *fused, 0.005, t, zflags=None if zf is None else T(zf))
            grad = ops.spmm_flagged(A, T(X), None, 0.25, 1.0, T(Zp), None if zf is None else T(zf))
            ops.adam_dense(*([pair[0], grad] + pair[1:]), 0.005, t)
            g64 = 0.25 * (g['M'] @ X.astype(np.float64)) + Z.astype(np.float64) * (1 if zf is None else zf[:, None])
            r64 = list(adam64(r64[0], g64, r64[1], r64[2], 0.005, t))
            for got, want, want64 in zip(fused, pair, r64):
                assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < RTOL
                assert rel_err(got.cpu().numpy(), want64) < RTOL


def only_set(A, k):
    """The same graph with a plan of row set k alone: one launch of the blocked kernel (+ its split-row combine)."""
    B = copy.copy(A)
    B.blocked = copy.copy(A.blocked)
    B.blocked.sets = [A.blocked.sets[k]]
    return B


@case
def test_rows_of_the_other_set_are_not_written(ops, U, I, rpw, unroll, d):
    g = graph(ops, U, I, rpw, unroll)
    A, N = g['A'], g['N']
    X, Z = inputs(g, d, 29 + d)
    zf = flags(g, 'alternating')
    rng = np.random.default_rng(31)
    P = rng.standard_normal((N, d)).astype(np.float32) * 0.1
    M = rng.standard_normal((N, d)).astype(np.float32) * 0.01
    V = rng.random((N, d)).astype(np.float32) * 1e-4 + 1e-6
    full_y = ops.spmm_flagged(A, T(X), None, 0.5, 0.25, T(Z), T(zf))
    full_s = T(Z); full_ys = torch.empty_like(full_s)
    ops.spmm_layersum(A, T(X), T(Z), full_s, full_ys)
    full_pmv = [T(P), T(M), T(V)]
    ops.spmm_adam(A, T(X), 0.25, 1.0, T(Z), *full_pmv, 0.005, 7, zflags=T(zf))
    for k, (lo, hi) in enumerate(((0, U), (U, N))):
        B = only_set(A, k)
        inside = torch.zeros(N, dtype=torch.bool, device=DEV); inside[lo:hi] = True

        def check(got, full):
            assert torch.equal(got[inside], full[inside])
            assert bool((got[~inside] == SENTINEL).all())

        Y = torch.full((N, d), SENTINEL, device=DEV)
        ops.spmm_flagged(B, T(X), None, 0.5, 0.25, T(Z), T(zf), out=Y)
        check(Y, full_y)
        Y = torch.full((N, d), SENTINEL, device=DEV)
        bits = T(np.full((N + 31) // 32, -1, np.int32))
        ops.spmm_flagged(B, T(X), bits, 0.5, 0.25, T(Z), T(zf), out=Y)      # masked build
        check(Y, full_y)
        S = torch.full((N, d), SENTINEL, device=DEV); Ys = torch.full((N, d), SENTINEL, device=DEV)
        ops.spmm_layersum(B, T(X), T(Z), S, Ys)
        check(S, full_s); check(Ys, full_ys)
        pmv = [torch.where(inside[:, None], T(t), torch.full((N, d), SENTINEL, device=DEV)) for t in (P, M, V)]
        ops.spmm_adam(B, T(X), 0.25, 1.0, T(Z), *pmv, 0.005, 7, zflags=T(zf))
        for got, full in zip(pmv, full_pmv):
            check(got, full)

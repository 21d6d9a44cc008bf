"""The fp16 split of score_mask_topk, restated in numpy (tests/topk_split_restatement.py), against the contract that the kernels' comment and
ops.score_mask_topk state:  |score - float64| <= gamma_d |a| |b|,  gamma_d = d 2^-24 + 2^-21,  and lists that differ from float64's only by near-ties.
No GPU: this is the evidence the device gate of the split path (kSplitSpreadLog2 = 16, the clamp of split_scale) rests on."""
import numpy as np
import pytest

import topk_split_restatement as R


def _tables(rng, d, U=300, I=2000):
    return (rng.normal(size=(U, d)) * 0.1).astype(np.float32), (rng.normal(size=(I, d)) * 0.1).astype(np.float32)


def _pin_max(X, m=0.25):
    """The table rescaled so that its largest magnitude is exactly m, a power of two: its scaled maximum is 2^13, the low end of [2^13, 2^14)."""
    X = (X / np.abs(X).max() * m).astype(np.float32)
    X.flat[np.abs(X).argmax()] = m
    return X


def _edge_tables(rng, d, G, n=300):
    """Worst case INSIDE a spread of 2^G.  A: a table whose maximum is 2^-2 exactly (row 0), a third of its rows i.i.d. and rescaled so that each row's largest
    element is 2^-G of that, a third 'spiked': one element at 2^-G of the maximum, all others odd multiples of 2^-25 in the scaled domain -- half-way
    points of the subnormal fp16 grid, where the low piece's rounding error is its largest, 2^-25 ABSOLUTE.  B: ordinary rows, plus for every spiked row
    one row of constant magnitude whose signs follow that row's rounding residuals, so that the 2^-25 errors add up coherently: the pair's error is
    sqrt(d) 2^(G-38) |a||b|, the bound the gate's constant is derived from."""
    A = _pin_max((rng.normal(size=(n, d)) * 0.1).astype(np.float32))
    A[0, 0] = 0.25
    a, b = np.arange(1, n // 3), np.arange(n // 3, 2 * n // 3)
    A[a] = (A[a] / np.abs(A[a]).max(axis=1, keepdims=True) * 0.25 * 2.0 ** -G).astype(np.float32)
    unit = 2.0 ** -25 / R.split_scale(0.25)
    A[b] = (unit * (2 * rng.integers(0, 4, size=(len(b), d)) + 1) * rng.choice([-1.0, 1.0], size=(len(b), d))).astype(np.float32)
    A[b, rng.integers(0, d, len(b))] = 0.25 * 2.0 ** -G
    h, l, s = R.split_pieces(A)
    resid = A.astype(np.float64) * s - h - l
    B = _pin_max((rng.normal(size=(2 * n, d)) * 0.1).astype(np.float32))
    B[n:n + len(b)] = np.where(resid[b] >= 0, 0.2, -0.2).astype(np.float32)
    return A, B


def test_split_scale_and_its_clamp():
    """split_scale brings a table's largest magnitude into [2^13, 2^14) exactly for exponents -27 .. 53; past them the scale stops at 2^+-40; 1 for
    zero, subnormal and non-finite maxima."""
    for e in range(-60, 80):
        for m in (1.0, 1.5, 1.9999999):
            x = np.float32(m * 2.0 ** e)
            sx = float(x) * R.split_scale(x)
            assert (2.0 ** 13 <= sx < 2.0 ** 14) == (R.EXP_LO <= e <= R.EXP_HI), (e, m)
            assert 2.0 ** -40 <= R.split_scale(x) <= 2.0 ** 40
    assert R.split_scale(np.float32(2.0 ** -28)) == 2.0 ** 40 and R.split_scale(np.float32(2.0 ** 54)) == 2.0 ** -40
    for x in (0.0, 1e-40, np.inf, np.nan):
        assert R.split_scale(np.float32(x)) == 1.0
    X = np.zeros((4, 8), np.float32)
    assert R.table_in_contract(X)                                   # all-zero: exact zeros
    X[1, 3] = 3.0
    assert R.table_in_contract(X)                                   # zero rows do not count
    X[2, 0] = 3.0 * 2.0 ** -16
    assert R.table_in_contract(X)
    X[2, 0] = 2.9 * 2.0 ** -16
    assert not R.table_in_contract(X)
    assert R.table_in_contract(np.full((2, 4), 2.0 ** -27, np.float32)) and not R.table_in_contract(np.full((2, 4), 1.9 * 2.0 ** -28, np.float32))
    assert R.table_in_contract(np.full((2, 4), 1.9 * 2.0 ** 53, np.float32)) and not R.table_in_contract(np.full((2, 4), 2.0 ** 54, np.float32))


@pytest.mark.parametrize('d', [64, 128])
def test_split_keeps_the_bound_inside_the_gate(d):
    """Inside the gate -- every nonzero row's largest |element| within 2^-16 of its table's, table exponents inside the clamp -- the restatement stays
    within gamma_d / 2 per pair (a 2x margin: the kernel's fp32 summation comes on top) and its lists differ from float64's by near-ties only.

    G = 16 is the largest spread with that margin.  Restatement, max |score - float64| / (|a||b|) over pairs, as a share of gamma_d:
      i.i.d. 0.1 N(0,1) tables, half of one table's rows scaled by 2^-s (users / items alike):
        d = 64 :  s <= 12: 0.014   s = 14: 0.017   s = 16: 0.049   s = 18: 0.21   s = 20: 0.85   s = 24: 13   s = 28: 190   s = 32: 3200
        d = 128:  s <= 12: 0.005   s = 14: 0.007   s = 16: 0.019   s = 18: 0.07   s = 20: 0.62   s = 24: 4.4  s = 28: 78    s = 32: 1100
      worst case at a spread of exactly 2^G (_edge_tables: spiked rows against sign-coherent items; sqrt(d) 2^(G-38) by derivation):
        d = 64 :  G = 14: 0.11   G = 15: 0.22   G = 16: 0.44   G = 17: 0.89
        d = 128:  G = 14: 0.08   G = 15: 0.17   G = 16: 0.33   G = 17: 0.67
    Random tables would allow 18; the worst case allows 16, and a gate has to hold in the worst case.  (fp32 dot product, same inputs: 0.05 gamma_d.)"""
    g = R.gamma(d)
    assert R.SPREAD_LOG2 == 16
    worst = {}
    for s in (0, 8, 12, 14):
        rng = np.random.default_rng(10 * d + s)
        Pu, Pi = _tables(rng, d)
        small = Pu.copy(); small[1::2] *= np.float32(2.0 ** -s)
        assert R.table_in_contract(small) and R.table_in_contract(Pi)
        worst['s=%d' % s] = max(R.pair_error(R.split_scores(small, Pi), small, Pi), R.pair_error(R.split_scores(Pi, small), Pi, small))
    rng = np.random.default_rng(d)
    A, B = _edge_tables(rng, d, 16)
    assert R.table_in_contract(A) and R.table_in_contract(B)
    worst['edge users'] = R.pair_error(R.split_scores(A, B), A, B)
    worst['edge items'] = R.pair_error(R.split_scores(B, A), B, A)
    assert worst['edge users'] > 0.25 * g                           # (the construction does reach the derived worst case: 0.44 / 0.33 of gamma_d)
    for e in (R.EXP_LO, R.EXP_HI):                                  # the ends of the clamp: the whole table moved there by an exact power of two
        Pu, Pi = _tables(rng, d)
        Pu[1::2] *= np.float32(2.0 ** -12)
        Pu = _pin_max(Pu, 2.0 ** e if e == R.EXP_LO else 1.99 * 2.0 ** e)
        assert R.table_in_contract(Pu)
        worst['exponent %d' % e] = R.pair_error(R.split_scores(Pu, Pi), Pu, Pi)
    print({k: '%.3f gamma' % (v / g) for k, v in worst.items()})
    assert max(worst.values()) <= 0.5 * g, worst
    # the list rule, on the case the device tests use at the edge of the gate: small rows on either side
    for side in (0, 1):
        Pu, Pi = _tables(rng, d)
        (Pu, Pi)[side][1::2] *= np.float32(2.0 ** -12)
        ref, ridx = R.reference_topk(Pu, Pi, 50)
        sc = R.split_scores(Pu, Pi)
        idx = R.stable_topk(sc, 50)
        R.check_lists(idx, np.take_along_axis(sc, idx, 1).astype(np.float32), ref, ridx, Pu, Pi, g)


@pytest.mark.parametrize('d', [64, 128])
def test_split_breaks_the_bound_past_the_gate(d):
    """Past the gate the split does NOT keep the contract -- which is why those tables take the exact fp32 build: one step past the spread the margin is
    gone (worst case at 2^17: 0.89 / 0.67 of gamma_d), rows at 2^-24 of their table break the value bound outright (13 / 4.4 gamma_d), rows at 2^-32
    break the list rule (150 to 180 items of 300 lists lost that are no near-ties; 10 at d = 128 with small items).  Outside the clamp the decay is
    slower, because the whole table shrinks together: an ordinary table at 2^-45 sits 2^-20 below [2^13, 2^14), its low pieces are all subnormal and the
    restatement is at 0.82 / 0.31 of gamma_d over all pairs (50 times an ordinary table's figure, no margin left at d = 64, lists still right); at 2^-60
    the high pieces go too and every list is wrong (2 500 items lost).  The gate sits at the clamp's ends all the
    same: inside them the scale is exact by construction, outside nothing is promised."""
    g = R.gamma(d)
    rng = np.random.default_rng(7 * d)
    A, B = _edge_tables(rng, d, 17)
    assert not R.table_in_contract(A)
    assert R.pair_error(R.split_scores(A, B), A, B) > 0.5 * g
    for side in (0, 1):
        Pu, Pi = _tables(rng, d)
        (Pu, Pi)[side][1::2] *= np.float32(2.0 ** -24)
        assert not R.table_in_contract((Pu, Pi)[side])
        assert R.pair_error(R.split_scores(Pu, Pi), Pu, Pi) > 2 * g
    lost = {}
    for name in ('small users', 'small items', 'table at 2^-45', 'table at 2^-60'):
        Pu, Pi = _tables(rng, d)
        if name == 'small users':
            Pu[1::2] *= np.float32(2.0 ** -32)
        elif name == 'small items':                                  # users along -e1 against large items with a positive first coordinate: their lists are small items only
            Pi[:, 0] = np.abs(Pi[:, 0]) + 0.3
            Pi[1::2] *= np.float32(2.0 ** -32)
            Pu[:, 0] = -np.abs(Pu[:, 0]) - 0.3
        else:
            Pu *= np.float32(2.0 ** (-45 if '45' in name else -60))
        assert not (R.table_in_contract(Pu) and R.table_in_contract(Pi))
        ref, ridx = R.reference_topk(Pu, Pi, 50)
        sc = R.split_scores(Pu, Pi)
        idx = R.stable_topk(sc, 50)
        f = R.list_figures(idx, np.take_along_axis(sc, idx, 1).astype(np.float32), ref, ridx, Pu, Pi, g)
        if name == 'table at 2^-45':
            f['worst'] = R.pair_error(sc, Pu, Pi) / g                # (over ALL pairs, as in the other error figures)
        lost[name] = (f['lost'], round(f['worst'], 2))
    print(lost)
    assert lost['small users'][0] > 0 and lost['small items'][0] > 0 and lost['table at 2^-60'][0] > 0, lost
    assert lost['table at 2^-45'][1] > 0.2, lost                     # (an ordinary table: 0.015 / 0.005)

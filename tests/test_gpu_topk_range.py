"""score_mask_topk on tables whose rows differ WIDELY in size -- near-dead users, freshly injected items, one outlier element, whole tables at
2^+-24 or 2^-45 -- against the contract ops.score_mask_topk states: for every returned pair |val - float64 score| <= gamma_d |a_u| |b_i|,
gamma_d = d 2^-24 + 2^-21, and lists that differ from float64's only by near-ties (tests/topk_split_restatement.py: check_lists).

The default path cuts every element of a table into two fp16 pieces after ONE power-of-two scale per table, which keeps that bound only for rows
within 2^-16 of their table's largest element and table exponents in [-27, 53] (tests/test_topk_split_cpu.py); past that the device routes the
call to the exact fp32 build.  Every case here runs every variant -- cold and warm-started from its own result, norm-ordered and table-ordered
stream, both forms of the stream at d = 64 -- which must agree bit for bit, and asserts the route the device took (ops.topk_fallbacks).
Reference: float64 matmul, stable descending order (ties: lowest item id first)."""
import functools

import numpy as np
import pytest
import torch

import topk_split_restatement as R

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = 300
SHAPES = [(64, 2000), (64, 40000), (128, 40000)]     # the short stream runs cold with no bootstrap; the long ones have the bootstrap, the norm order and the exit gate
KS = (20, 50)
SPLIT, EXACT = False, True                           # routes, as ops.topk_fallbacks reports them


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on the MI355X box)')
    from arlib_amd import ops as _ops
    return _ops


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def _base_tables(d, I, n_users=U):
    rng = np.random.default_rng(1000 * d + I + n_users)
    Pu, Pi = (rng.normal(size=(n_users, d)) * 0.1).astype(np.float32), (rng.normal(size=(I, d)) * 0.1).astype(np.float32)
    Pu.setflags(write=False); Pi.setflags(write=False)
    return Pu, Pi


def _tables(d, I, n_users=U):
    Pu, Pi = _base_tables(d, I, n_users)
    return Pu.copy(), Pi.copy()


def _e1_geometry(Pu, Pi):
    """Every item gets a positive first coordinate, a third of the users point along -e1, the others get a positive one: whatever the items' sizes, the
    -e1 users score every item below zero -- the SMALLEST items best -- and the others rank by size."""
    Pi[:, 0] = np.abs(Pi[:, 0]) + np.float32(0.3)
    Pu[:, 0] = np.abs(Pu[:, 0])
    Pu[1::3] *= np.float32(0.2)
    Pu[1::3, 0] = -np.abs(Pu[1::3, 0]) - np.float32(0.5)


def _mask_of_best(ref, rng, rows_with_best):
    """Per user: 20 random items and, for the given rows (and every third of the others), the user's 5 .. 30 best items by float64."""
    best = R.stable_topk(ref, 30)
    cols = []
    for u in range(ref.shape[0]):
        n_best = int(rng.integers(5, 31)) if (u in rows_with_best or u % 3 == 0) else 0
        cols.append(np.unique(np.concatenate([best[u, :n_best], rng.choice(ref.shape[1], size=20, replace=False)])).astype(np.int32))
    return cols


def _run_variants(ops, Pu, Pi, k, rp, mc, d):
    """[(name, idx, val)] of every variant of the default path, and the route of each call."""
    tPu, tPi = T(Pu), T(Pi)
    out = []
    saved = ops.TOPK_STATS.get('record_route', False)
    ops.TOPK_STATS['record_route'], ops.TOPK_STATS['route'] = True, []
    try:
        for form2 in ((True, False) if d == 64 else (True,)):
            ops.TOPK_FORM2 = form2
            ops.reset_exit_probe()
            for order in ('norm', None):
                i_c, v_c = ops.score_mask_topk(tPu, tPi, k, rp, mc, item_order=order)
                i_w, v_w = ops.score_mask_topk(tPu, tPi, k, rp, mc, item_order=order, warm_idx=i_c)
                out += [('form2=%s order=%s cold' % (form2, order), i_c, v_c), ('form2=%s order=%s warm' % (form2, order), i_w, v_w)]
        routes = ops.topk_fallbacks()
    finally:
        ops.TOPK_FORM2 = True
        ops.TOPK_STATS['record_route'] = saved
        ops.reset_exit_probe()
    return out, routes


def _check_case(ops, name, Pu, Pi, d, route, cols=None, exact_too=False, ks=KS):
    """One case at every k: inputs fit for the check (an fp32 numpy matmul stays under the near-tie cap), all variants bit-identical, the contract, the route."""
    assert (R.table_in_contract(Pu) and R.table_in_contract(Pi)) == (route == SPLIT), 'the case is on the wrong side of the gate'
    ref, ridx = R.reference_topk(Pu, Pi, max(ks), cols)
    sc32 = (Pu @ Pi.T).astype(np.float64)
    if cols is not None:
        for u, c in enumerate(cols):
            sc32[u, c] = -10e8
    assert (R.stable_topk(sc32, max(ks)) != ridx).mean() <= 0.005, 'inputs: near-ties all over, the list check would excuse too much'
    del sc32
    rp = mc = None
    if cols is not None:
        rp = T(np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)); mc = T(np.concatenate(cols))
    g = R.gamma(d)
    first = {}
    for k in ks:
        variants, routes = _run_variants(ops, Pu, Pi, k, rp, mc, d)
        _, i0, v0 = variants[0]
        for vname, i_x, v_x in variants[1:]:
            assert torch.equal(i_x, i0) and torch.equal(v_x, v0), '%s k=%d: %s differs from %s' % (name, k, vname, variants[0][0])
        idx, val = i0.cpu().numpy(), v0.cpu().numpy()
        f = R.list_figures(idx, val, ref, ridx[:, :k], Pu, Pi, g)
        print('%s d=%d I=%d k=%d: %s routes(exact)=%s' % (name, d, Pi.shape[0], k, f, sorted(set(routes))))
        R.check_lists(idx, val, ref, ridx[:, :k], Pu, Pi, g)
        assert routes == [route] * len(variants), routes
        if exact_too:                                               # the build the gate routes to, asked for directly: the fp32 dot-product bound alone
            i_e, v_e = ops.score_mask_topk(T(Pu), T(Pi), k, rp, mc, exact=True)
            R.check_lists(i_e.cpu().numpy(), v_e.cpu().numpy(), ref, ridx[:, :k], Pu, Pi, d * 2.0 ** -24)
        first[k] = (idx, val)
    return ref, ridx, first


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('s', [12, 24, 32])
@pytest.mark.parametrize('d,I', SHAPES)
def test_small_user_rows(ops, d, I, s, masked):
    """A third of the users at 2^-s of the rest (row 0 keeps the table's maximum).  Masked: the small users' interacted items include their best ones.
    2^-12 is inside the split's contract, 2^-24 and 2^-32 take the exact build.
    BEFORE the gate (the split on every table; one run on an MI355X, one cold call per case, k = 50; worst returned pair as a multiple of gamma_d /
    items lost that are no near-ties / share of the 15 000 list positions that differ from float64's):
        small users   d = 64, I = 2000:   s = 12: 0.017 / 0 / 0     s = 24:  9.5 / 0 / 0.3 %    s = 32: 2309 / 124 / 21 %
                      d = 64, I = 40000:  s = 12: 0.023 / 0 / 0     s = 24: 12.2 / 1 / 0.3 %    s = 32: 2746 / 164 / 24 %
                      d = 128, I = 40000: s = 12: 0.010 / 0 / 0     s = 24:  3.9 / 0 / 0.2 %    s = 32: 1025 / 165 / 24 %
        small items   d = 64, I = 2000:   s = 12: 0.043 / 0 / 0     s = 24: 12.3 / 2 / 1.1 %    s = 32: 3248 / 556 / 31 %
        (test below)  d = 64, I = 40000:  s = 12: 0.045 / 0 / 0     s = 24: 12.7 / 2 / 1.8 %    s = 32: 3155 / 909 / 31 %
                      d = 128, I = 40000: s = 12: 0.018 / 0 / 0     s = 24:  5.1 / 1 / 0.9 %    s = 32: 1346 / 679 / 30 %
    -- the numpy restatement's decay (tests/test_topk_split_cpu.py), confirmed on the device.  With the gate every case is below 0.07 gamma_d."""
    Pu, Pi = _tables(d, I)
    small = np.arange(1, U, 3)
    Pu[small] *= np.float32(2.0 ** -s)
    cols = None
    if masked:
        ref = Pu.astype(np.float64) @ Pi.astype(np.float64).T
        cols = _mask_of_best(ref, np.random.default_rng(s), set(small.tolist()))
    _check_case(ops, 'small users 2^-%d%s' % (s, ' masked' if masked else ''), Pu, Pi, d, SPLIT if s == 12 else EXACT, cols, exact_too=True)


def test_small_user_rows_ragged_last_workgroup_of_the_second_form(ops):
    """1 300 users = 2 x 512 + 276 at d = 64, small rows inside the contract: the second form's last workgroup is ragged, and the call stays on the split."""
    d, I = 64, 40000
    Pu, Pi = _tables(d, I, 1300)
    Pu[1::3] *= np.float32(2.0 ** -12)
    _check_case(ops, 'small users 2^-12, 1300 users', Pu, Pi, d, SPLIT, ks=(50,))


@pytest.mark.parametrize('s', [12, 24, 32])
@pytest.mark.parametrize('d,I', SHAPES)
def test_small_item_rows(ops, d, I, s):
    """Half of the items at 2^-s of the rest.  The large items all have a positive first coordinate and a third of the users point along -e1: their
    lists are small items ONLY -- scores 2^-s of everybody else's, which the split resolves no better than the LARGE items' scale allows -- and the
    other users' lists are large items only."""
    Pu, Pi = _tables(d, I)
    _e1_geometry(Pu, Pi)
    Pi[1::2] *= np.float32(2.0 ** -s)
    _, ridx = R.reference_topk(Pu, Pi, max(KS))
    assert (ridx[1::3] % 2 == 1).all() and (ridx[0::3] % 2 == 0).all() and (ridx[2::3] % 2 == 0).all()       # small items only / large items only
    _check_case(ops, 'small items 2^-%d' % s, Pu, Pi, d, SPLIT if s == 12 else EXACT, exact_too=True)


@pytest.mark.parametrize('d,I', SHAPES)
def test_small_users_against_small_items(ops, d, I):
    """Both at once, 2^-24 on each side: the -e1 users are the small users and their lists are the small items -- scores at 2^-48 of the largest."""
    Pu, Pi = _tables(d, I)
    _e1_geometry(Pu, Pi)
    Pu[1::3] *= np.float32(2.0 ** -24)
    Pi[1::2] *= np.float32(2.0 ** -24)
    _, ridx = R.reference_topk(Pu, Pi, max(KS))
    assert (ridx[1::3] % 2 == 1).all() and (ridx[0::3] % 2 == 0).all()
    _check_case(ops, 'small users x small items 2^-24', Pu, Pi, d, EXACT, exact_too=True)


@pytest.mark.parametrize('table', ['users', 'items'])
@pytest.mark.parametrize('d,I', SHAPES)
def test_one_outlier_element(ops, d, I, table):
    """Ordinary tables but for ONE element at 2^20 times the rest: every row but one is 'small' next to its table's maximum."""
    Pu, Pi = _tables(d, I)
    (Pu if table == 'users' else Pi)[5, 7] = np.float32(0.1 * 2.0 ** 20)
    _check_case(ops, 'outlier element in the %s' % table, Pu, Pi, d, EXACT)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('d,I', SHAPES)
def test_power_of_two_equivariance(ops, d, I, masked):
    """Pu * 2^p and Pi * 2^q, inside the clamp: scaling by a power of two is exact and the split rescales by powers of two, so the indices are the
    unscaled call's and the values are its values times 2^(p+q), bit for bit, on the split path -- anything else is an absolute constant that leaked
    into the scaled domain (the -1e-30 of the warm bound, the pre-filter's absolute term, the -10e8 mask key)."""
    Pu, Pi = _tables(d, I)
    cols = None
    if masked:
        cols = _mask_of_best(Pu.astype(np.float64) @ Pi.astype(np.float64).T, np.random.default_rng(d + I), set())
    ref, ridx, base = _check_case(ops, 'unscaled%s' % (' masked' if masked else ''), Pu, Pi, d, SPLIT, cols)
    for p, q in ((-24, 0), (0, 24), (12, -24), (24, 24)):
        Su, Si = Pu * np.float32(2.0 ** p), Pi * np.float32(2.0 ** q)
        _, _, got = _check_case(ops, 'scaled by 2^%d, 2^%d%s' % (p, q, ' masked' if masked else ''), Su, Si, d, SPLIT, cols)
        for k in KS:
            assert np.array_equal(got[k][0], base[k][0]), (p, q, k)
            assert np.array_equal(got[k][1], base[k][1] * np.float32(2.0 ** (p + q))), (p, q, k)


@pytest.mark.parametrize('p,q', [(-45, 0), (0, -45)])
@pytest.mark.parametrize('d,I', SHAPES)
def test_table_outside_the_clamp(ops, d, I, p, q):
    """A whole table at 2^-45: its largest magnitude has an exponent below -27, where split_scale stops short of [2^13, 2^14).  The exact build takes it."""
    Pu, Pi = _tables(d, I)
    _check_case(ops, 'tables at 2^%d, 2^%d' % (p, q), Pu * np.float32(2.0 ** p), Pi * np.float32(2.0 ** q), d, EXACT)


@pytest.mark.parametrize('kind', ['zero users', 'zero items', 'zero rows', 'single element'])
@pytest.mark.parametrize('d,I', SHAPES)
def test_degenerate_tables(ops, d, I, kind):
    """All-zero tables, zero rows inside ordinary tables, a table with a single nonzero element: values are exact zeros where float64's are (check_lists
    allows no error at all against a zero row), zero scores tie in table order -- lowest item id first, np.argsort(kind='stable') on the reference --
    and no NaN appears.  Zero rows do not count towards the spread: all of these stay on the split."""
    Pu, Pi = _tables(d, I)
    if kind == 'zero users':
        Pu[:] = 0
    elif kind == 'zero items':
        Pi[:] = 0
    elif kind == 'zero rows':
        Pu[0] = 0; Pu[77] = 0; Pu[U - 1] = 0; Pi[0] = 0; Pi[1001] = 0; Pi[I - 1] = 0
    else:
        Pu[:] = 0; Pu[3, 5] = np.float32(0.7)
    ref, ridx, got = _check_case(ops, kind, Pu, Pi, d, SPLIT)
    for k in KS:
        idx, val = got[k]
        r = np.take_along_axis(ref, idx.astype(np.int64), 1)
        assert (val[r == 0] == 0).all()
        allzero = ~ref.any(axis=1)
        assert allzero.sum() == {'zero users': U, 'zero items': U, 'zero rows': 3, 'single element': U - 1}[kind]
        assert (idx[allzero] == np.arange(k)[None, :]).all()        # ties in table order
        assert np.array_equal(idx[allzero], ridx[allzero, :k])


@pytest.mark.parametrize('d', [64, 128])
def test_gate_hangs_on_one_element_anywhere(ops, d):
    """The gate's input is the smallest nonzero row maximum of each table, reduced on the device over every row and column: one row of either table is
    zero but for ONE element at exactly 2^-16 of its table's largest (inside the contract: split, and the bound holds at the very edge of the gate) or
    1 % below (outside: exact build) -- at the first and last row and column and in between (rows share a wave with 1 or 3 others)."""
    I = 2000
    for table in ('users', 'items'):
        n = U if table == 'users' else I
        for r, c in ((0, 0), (1, 5), (17, d // 2 - 1), (n // 2, 16), (n - 1, d - 1)):
            for inside in (True, False):
                Pu, Pi = _tables(d, I)
                X = Pu if table == 'users' else Pi
                m = np.abs(X).max()
                assert np.abs(X[r]).max() < m
                X[r] = 0
                X[r, c] = m * np.float32(2.0 ** -16) * np.float32(1.0 if inside else 0.99)
                _check_case(ops, 'edge %s[%d, %d] %s' % (table, r, c, 'inside' if inside else 'outside'), Pu, Pi, d, SPLIT if inside else EXACT, ks=(20,))

"""GOAT on the CPU (the library's host entries run here): the native itemSample against the reference's captured calls (g32,
tests/golden/gen_golden_goat.py), the bound up to which it is exact and the Python route past it against the reference's literal set
expression, the constructor's co-rating degree and the initial parameters, the errors, the range checks of the co-rating kernel's entry (they
precede every device call), and arl_goat_item_sample under AddressSanitizer / UBSan as a stand-alone program."""
import hashlib
import os
import random
import shutil
import subprocess
import sys
import warnings

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from conftest import golden, ROOT
from test_host_api import make_data

KS = (46, 100, 300)


def state_sha():
    return hashlib.sha256(np.frombuffer(repr(random.getstate()).encode(), np.uint8).tobytes()).hexdigest()


@pytest.fixture(scope='module')
def ml100k():
    """(g32, CSR of the training matrix, itemIntNum from the host expression)."""
    from arlib_amd import corating
    X = sp.csr_matrix(make_data().matrix())
    X.sort_indices()
    return golden('g32_goat.npz'), X, corating.corating_degree_host(X)


def literal_item_sample(X, int_num, targets, F, k, O_u, O_i):
    """itemSample as the reference states it: dense rows, lists of floats, and random.sample of the SET difference (what only Python < 3.11 runs)."""
    U, I = X.shape
    cnt, thr = [float(v) for v in int_num], int(O_i * U)
    user = np.zeros((1, I))
    rows_s, rows_f, rows_real = [], [], []
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)
        for _ in range(F):
            s, f = [], []
            while user.sum() < O_u * I:
                user = X[random.randint(0, U - 1), :].toarray()[0, :]
            for j in user.nonzero()[0].tolist():
                if cnt[j] > thr and len(s) < int(k * 0.3):
                    s.append(j)
                elif cnt[j] > thr / 3 and len(f) < int(k * 0.7):
                    f.append(j)
            while len(s) < int(k * 0.3):
                s += random.sample(set(list(range(I))) - set(targets) - set(s) - set(f), int(k * 0.3) - len(s))
            while len(f) + len(s) < k:
                f += random.sample(set(list(range(I))) - set(targets) - set(s) - set(f), k - len(f) - len(s))
            rows_s.append(s); rows_f.append(f); rows_real.append(user[s + f])
    return np.array(rows_s, np.int32).reshape(F, -1), np.array(rows_f, np.int32).reshape(F, -1), np.array(rows_real).astype(np.uint8)


def synthetic(U, I, seed, heavy):
    """A 0/1 matrix whose user 0 has `heavy` items, with item degrees that spread over the thresholds."""
    rng = np.random.RandomState(seed)
    D = (rng.random_sample((U, I)) < np.linspace(0.02, 0.5, I)[None, :]).astype(np.float32)
    D[0] = 0
    D[0, rng.choice(I, heavy, replace=False)] = 1
    X = sp.csr_matrix(D)
    X.sort_indices()
    return X


# ---------------------------------------------------------------------------------------------------- the sampler against g32
@pytest.mark.parametrize('k', KS)
def test_native_sampler_reproduces_the_reference(ml100k, k):
    from arlib_amd.attack.Gray import GOAT as M
    g, X, int_num = ml100k
    U, I = X.shape
    assert M.native_sampling_exact(k, len(g['targets']), I)
    random.seed(11)
    for call in range(4):
        I_s, I_f, real, user = M.item_sample(X.indptr, X.indices, U, I, int_num, g['targets'], 9, k, 0.01, 0.02)
        assert I_s.shape == (9, int(k * 0.3)) and I_f.shape == (9, k - int(k * 0.3)) and real.shape == (9, k) and real.dtype == np.uint8
        assert np.array_equal(I_s, g['samp%d_Is' % k][call]) and np.array_equal(I_f, g['samp%d_If' % k][call])
        assert np.array_equal(real, g['samp%d_real' % k][call])
        assert state_sha() == str(g['samp%d_state_sha' % k][call])
        assert X[user].nnz >= 0.01 * I and np.array_equal(real, np.isin(np.concatenate([I_s, I_f], 1), X[user].indices))


@pytest.mark.parametrize('k', KS)
def test_python_route_reproduces_the_reference_too(ml100k, k):
    from arlib_amd.attack.Gray import GOAT as M
    g, X, int_num = ml100k
    random.seed(11)
    for call in range(2):
        I_s, I_f, real, _ = M.item_sample_python(X.indptr, X.indices, X.shape[0], X.shape[1], int_num, g['targets'], 9, k, 0.01, 0.02)
        assert np.array_equal(I_s, g['samp%d_Is' % k][call]) and np.array_equal(I_f, g['samp%d_If' % k][call])
        assert np.array_equal(real, g['samp%d_real' % k][call]) and state_sha() == str(g['samp%d_state_sha' % k][call])


def test_fixture_shows_the_fill_path_and_one_real_user_per_call(ml100k):
    """What the fixture has to contain for the tests above to mean something: rows of one call differ (the fill draws), share their walk prefix
    (one real user), and the real user lacks some candidates."""
    g = ml100k[0]
    for k in KS:
        Is, If, real = g['samp%d_Is' % k], g['samp%d_If' % k], g['samp%d_real' % k]
        assert any(not np.array_equal(If[c, 0], If[c, 1]) for c in range(4))
        assert all((real[c] == 0).any() for c in range(4))
        assert all(np.array_equal(Is[c, 0, :3], Is[c, f, :3]) for c in range(4) for f in range(9))


# ---------------------------------------------------------------------------------------------------- bound and fallback
def test_native_route_only_inside_the_bound(monkeypatch):
    from arlib_amd.attack.Gray import GOAT as M
    assert M.native_sampling_exact(46, 5, 1412) and M.native_sampling_exact(20, 5, 64) and M.native_sampling_exact(9, 5, 35)
    assert not M.native_sampling_exact(24, 5, 37) and not M.native_sampling_exact(10, 5, 37) and not M.native_sampling_exact(0, 5, 1412)
    assert M.native_sampling_exact(559, 5, 1412) and not M.native_sampling_exact(560, 5, 1412)         # 0.4 * 1412 = 564.8
    taken = []
    monkeypatch.setattr(M, 'item_sample_native', lambda *a: taken.append('native'))
    monkeypatch.setattr(M, 'item_sample_python', lambda *a: taken.append('python'))
    X = synthetic(6, 37, 1, 30)
    cnt = np.ones(37)
    M.item_sample(X.indptr, X.indices, 6, 37, cnt, [1, 2, 3, 4, 5], 3, 9, 0.5, 0.2)
    M.item_sample(X.indptr, X.indices, 6, 37, cnt, [1, 2, 3, 4, 5], 3, 10, 0.5, 0.2)
    assert taken == ['native', 'python']


def test_library_refuses_the_shape_past_the_bound():
    from arlib_amd import _lib
    from arlib_amd.attack.Gray import GOAT as M
    from arlib_amd import corating
    X = synthetic(6, 37, 1, 30)
    st = random.getstate()
    with pytest.raises(_lib.ArlError, match='ARL_E_RANGE'):
        M.item_sample_native(X.indptr, X.indices, 6, 37, corating.corating_degree_host(X), [1, 2, 3, 4, 5], 3, 24, 0.5, 0.2)
    assert random.getstate() == st


@pytest.mark.skipif(sys.version_info >= (3, 11), reason='random.sample of a set raises from Python 3.11 on: the literal expression cannot run')
def test_fallback_equals_the_literal_expression_where_the_set_is_not_ascending():
    """I = 37 with 29 ids removed: the tuple of the set difference is not ascending, the native sampler's premise fails, the wrapper's route is exact."""
    from arlib_amd.attack.Gray import GOAT as M
    from arlib_amd import corating
    X = synthetic(6, 37, 1, 30)
    cnt = corating.corating_degree_host(X)
    targets = [0, 9, 17, 30, 36]
    rest = tuple(set(list(range(37))) - set(targets) - set(range(1, 25)))
    assert list(rest) != sorted(rest)                                          # the premise of this test
    for seed in (3, 4):
        random.seed(seed)
        want = literal_item_sample(X, cnt, targets, 4, 24, 0.5, 10.0)
        after = random.getstate()
        random.seed(seed)
        got = M.item_sample(X.indptr, X.indices, 6, 37, cnt, targets, 4, 24, 0.5, 10.0)
        assert all(np.array_equal(a, b) for a, b in zip(want, got[:3])) and random.getstate() == after and got[3] == 0
    assert want[0].shape == (4, 7) and not np.array_equal(want[0][0], want[0][1])       # O_i = 10: nothing qualifies for I_s, every row draws its own


@pytest.mark.skipif(sys.version_info >= (3, 11), reason='random.sample of a set raises from Python 3.11 on: the literal expression cannot run')
@pytest.mark.parametrize('I,U,k,heavy,O_i', [(64, 8, 20, 40, 0.5), (64, 8, 20, 40, 10.0), (64, 8, 3, 12, 0.5), (1412, 0, 46, 0, 0.02), (1412, 0, 300, 0, 0.02)])
def test_native_equals_the_literal_expression_inside_the_bound(ml100k, I, U, k, heavy, O_i):
    """Both forms of random.sample are met: at I = 64 the pool of <= 59 ids is below CPython's set-size rule (the pool form), at 1 412 it is above."""
    from arlib_amd.attack.Gray import GOAT as M
    from arlib_amd import corating
    if I == 1412:
        g, X, cnt = ml100k
        targets, O_u = g['targets'].tolist(), 0.01
    else:
        X = synthetic(U, I, I + k, heavy)
        cnt, targets, O_u = corating.corating_degree_host(X), [3, 5, 8, 13, 21], 0.1
    F = 5
    assert M.native_sampling_exact(k, len(targets), I)
    random.seed(7)
    want = [literal_item_sample(X, cnt, targets, F, k, O_u, O_i) for _ in range(2)]
    after = random.getstate()
    random.seed(7)
    got = [M.item_sample_native(X.indptr, X.indices, X.shape[0], I, cnt, targets, F, k, O_u, O_i) for _ in range(2)]
    assert random.getstate() == after
    for w, gt in zip(want, got):
        assert all(np.array_equal(a, b) for a, b in zip(w, gt[:3]))


# ---------------------------------------------------------------------------------------------------- constructor data
def test_host_corating_degree_equals_the_reference(ml100k):
    g, X, int_num = ml100k
    assert int_num.dtype == np.float64 and np.array_equal(int_num, g['item_int_num'])
    D = X.toarray().astype(np.float64)
    assert np.array_equal(int_num, ((D.T @ D) > 0).sum(0))
    assert int_num.min() == 11.0 and int_num.max() == 1275.0


def test_initial_parameters_match_the_reference_bit_for_bit(ml100k):
    from arlib_amd.attack.Gray.GOAT import Encoder, Decoder
    g = ml100k[0]
    torch.manual_seed(int(g['seed']))
    G, D = Encoder(46), Decoder(46)
    names = ['G.' + n for n, _ in G.named_parameters()] + ['D.' + n for n, _ in D.named_parameters()]
    assert sorted('init_sha__' + n for n in names) == sorted(k for k in g.files if k.startswith('init_sha__')) and len(names) == 22
    for n, p in list(zip(names, list(G.parameters()) + list(D.parameters()))):
        assert hashlib.sha256(p.detach().numpy().astype(np.float32).tobytes()).hexdigest() == str(g['init_sha__' + n]), n


# ---------------------------------------------------------------------------------------------------- errors
def test_errors(ml100k):
    from arlib_amd.attack.Gray import GOAT as M
    g, X, cnt = ml100k
    U, I = X.shape
    a = (X.indptr, X.indices, U, I, cnt)
    st = random.getstate()
    for fn in (M.item_sample, M.item_sample_native, M.item_sample_python):
        with pytest.raises(ValueError, match='k == 0'):
            fn(*a, g['targets'], 9, 0, 0.01, 0.02)
        with pytest.raises(ValueError, match='no user has'):
            fn(*a, g['targets'], 9, 46, 0.9, 0.02)                              # nobody rated 90 % of the catalogue: the reference never returns
        with pytest.raises(ValueError, match='target item outside'):
            fn(*a, [3, I], 9, 46, 0.01, 0.02)
        with pytest.raises(ValueError, match='target item outside'):
            fn(*a, [-1], 9, 46, 0.01, 0.02)
    assert random.getstate() == st                                              # nothing was drawn


def test_library_checks_its_arguments_before_it_draws():
    from arlib_amd import _lib
    L = _lib.lib()
    from arlib_amd.util.sampler import MTState
    mt = MTState.from_seed(5).words
    rp, it, cnt, tg = np.array([0, 2], np.int64), np.array([0, 1], np.int32), np.ones(40), np.array([40], np.int32)
    outs = [np.zeros(64, np.int32) for _ in range(2)] + [np.zeros(64, np.uint8), np.zeros(1, np.int32), np.zeros(256, np.int32)]
    vp = lambda x: x.ctypes.data
    call = lambda k, targets, T: L.arl_goat_item_sample(vp(mt), vp(rp), vp(it), 1, 40, vp(cnt), vp(targets), T, 2, k, 1.0, 0, *[vp(o) for o in outs])
    assert call(4, tg, 1) == -4 and call(0, tg, 0) == -4 and call(16, tg, 0) == 0 and call(17, tg, 0) == -3
    assert L.arl_goat_item_sample(None, vp(rp), vp(it), 1, 40, vp(cnt), None, 0, 2, 4, 1.0, 0, *[vp(o) for o in outs]) == -1
    before = mt.copy()                                                          # the only user has 2 items: asking for 3 would draw forever
    assert L.arl_goat_item_sample(vp(mt), vp(rp), vp(it), 1, 40, vp(cnt), None, 0, 2, 4, 3.0, 0, *[vp(o) for o in outs]) == -4
    assert np.array_equal(mt, before)


def test_data_checked_once_gives_the_calls_of_the_raw_arguments(ml100k):
    """GOAT checks its CSR once in the constructor (SampleData) and samples 2 001 times on it: the same draws as the form that checks per call."""
    from arlib_amd.attack.Gray import GOAT as M
    g, X, cnt = ml100k
    U, I = X.shape
    data = M.SampleData(X.indptr, X.indices, U, I, cnt, g['targets'])
    assert data.max_degree == int(np.diff(X.indptr).max()) and data.items.dtype == np.int32 and data.rowptr.dtype == np.int64
    for fn in (M.item_sample, M.item_sample_native, M.item_sample_python):
        random.seed(5)
        a = fn(data, 9, 46, 0.01, 0.02)
        random.seed(5)
        b = fn(X.indptr, X.indices, U, I, cnt, g['targets'], 9, 46, 0.01, 0.02)
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match='item id outside'):
        M.SampleData(X.indptr, np.where(X.indices == 7, I, X.indices), U, I, cnt, g['targets'])
    with pytest.raises(ValueError, match='no user has'):
        M.item_sample(data, 9, 46, 0.9, 0.02)


def test_corating_entry_refuses_a_catalogue_past_its_bitmap_before_any_launch():
    from arlib_amd import _lib, corating
    L = _lib.lib()
    assert L.arl_corating_max_items() == corating.CORATING_MAX_ITEMS == (160 * 1024 - 64) * 8
    assert corating.corating_degree_supported(corating.CORATING_MAX_ITEMS) and not corating.corating_degree_supported(corating.CORATING_MAX_ITEMS + 1)
    one = np.zeros(4, np.int64)
    p = one.ctypes.data
    assert L.arl_corating_degree_i32(p, p, p, p, 2, corating.CORATING_MAX_ITEMS + 1, None, p, None) == -3
    assert L.arl_corating_degree_i32(p, p, p, p, 2 ** 31, 4, None, p, None) == -3
    assert L.arl_corating_degree_i32(p, p, p, p, -1, 4, None, p, None) == -4
    assert L.arl_corating_degree_i32(None, p, p, p, 2, 4, None, p, None) == -1
    assert L.arl_corating_degree_i32(None, None, None, None, 2, 0, None, None, None) == 0          # no items: nothing to do
    with pytest.raises(ValueError, match='corating_degree_host'):
        corating.corating_degree(np.zeros(3, np.int64), np.zeros(0, np.int32), 2, corating.CORATING_MAX_ITEMS + 1)


# ---------------------------------------------------------------------------------------------------- sanitizer
def test_item_sample_under_address_and_ub_sanitizer(ml100k, tmp_path):
    """arl_host.cpp and tests/goat_sample_main.cpp built with -fsanitize=address,undefined into a program of its own; it runs the fixture's
    twelve calls with buffers of exactly the documented sizes and must end clean with the fixture's values."""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx is not None, 'no host C++ compiler: the project cannot be built here either'
    # the sanitizer runtimes are linked INTO the program (clang does so by default), so it runs in the caller's environment as it is
    static = [] if 'clang' in os.path.basename(cxx) else ['-static-libasan', '-static-libubsan']
    g, X, cnt = ml100k
    U, I = X.shape
    exe, fin, fout = str(tmp_path / 'goat_sample_main'), str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
    subprocess.check_call([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all'] + static + ['-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'goat_sample_main.cpp'), os.path.join(ROOT, 'arlib_amd', 'csrc', 'arl_host.cpp'), '-o', exe])
    tg = g['targets'].astype(np.int32)
    with open(fin, 'wb') as fh:
        for a in (np.array([U, I, X.nnz, len(tg), 9, len(KS), 4, 11], np.int64), X.indptr.astype(np.int64), X.indices.astype(np.int32), cnt.astype(np.float64), tg,
                  np.array(KS, np.int64), np.array([0.01, 0.02], np.float64)):
            fh.write(a.tobytes())
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stderr == '', r.stderr[-2000:]
    buf, pos = open(fout, 'rb').read(), 0

    def take(dtype, *shape):
        nonlocal pos
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        a = np.frombuffer(buf, dtype, int(np.prod(shape)), pos).reshape(shape)
        pos += n
        return a
    for k in KS:
        random.seed(11)
        for call in range(4):
            s = int(k * 0.3)
            assert np.array_equal(take(np.int32, 9, s), g['samp%d_Is' % k][call]) and np.array_equal(take(np.int32, 9, k - s), g['samp%d_If' % k][call])
            assert np.array_equal(take(np.uint8, 9, k), g['samp%d_real' % k][call])
            take(np.int32, 1)
            mt = take(np.uint32, 625)
            st = random.getstate()
            random.setstate((st[0], tuple(int(x) for x in mt), st[2]))
            assert state_sha() == str(g['samp%d_state_sha' % k][call])
    assert pos == len(buf)

"""arlib_amd.neighbours, arlib_amd.detect and util.metrics.DetectionMetric without a GPU: the host route against the pure-Python restatement
(tests/cooccur_restatement.py), the wrapper's ValueErrors, the C entry's ARL_E_* codes (the library loads without a device and refuses before any
launch), DetectionMetric against hand-computed values and profile_features against direct numpy."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp

import cooccur_restatement as R

MEASURES = ('count', 'cosine', 'jaccard')


def random_matrix(n, I, density, seed):
    rng = np.random.RandomState(seed)
    D = (rng.random_sample((n, I)) < density).astype(np.int64)
    D[n // 3] = 0                                           # an empty row
    D[:, I // 2] = 0                                        # a column nobody has
    return sp.csr_matrix(D)


@pytest.fixture(scope='module')
def problems():
    out = {'random': random_matrix(70, 45, 0.15, 3), 'sparse': random_matrix(90, 200, 0.02, 4), 'identical': R.identical_rows(40, 36)}
    return {name: (X, {m: R.cooccur_topk(X, 64, m) for m in MEASURES}) for name, X in out.items()}


@pytest.mark.parametrize('measure', MEASURES)
@pytest.mark.parametrize('k', [1, 5, 64])
@pytest.mark.parametrize('name', ['random', 'sparse', 'identical'])
def test_host_route_equals_the_restatement(problems, name, k, measure):
    from arlib_amd import neighbours
    X, ref = problems[name]
    idx, cnt, deg = neighbours.cooccur_topk_host(X, k, measure)
    assert idx.dtype == np.int32 and cnt.dtype == np.int32 and deg.dtype == np.int64 and idx.shape == (X.shape[0], k)
    assert np.array_equal(idx, ref[measure][0][:, :k]) and np.array_equal(cnt, ref[measure][1][:, :k]) and np.array_equal(deg, ref[measure][2])
    if name == 'identical':                                 # every similarity ties: the smallest other ids, in order
        n = X.shape[0]
        for u in (0, 1, n - 1):
            assert idx[u].tolist() == ([v for v in range(n) if v != u][:k] + [-1] * k)[:k]
    assert np.array_equal(neighbours.similarity(idx, cnt, deg, None, measure), R.similarity(idx, cnt, deg, None, measure))


def test_host_route_rows_repeats_values_and_the_python_int_path(problems):
    from arlib_amd import neighbours
    X, ref = problems['random']
    rows = np.array([5, 69, 0, 5, 23], np.int64)
    for m in MEASURES:
        idx, cnt, _ = neighbours.cooccur_topk_host(X, 7, m, rows)
        assert np.array_equal(idx, ref[m][0][rows, :7]) and np.array_equal(cnt, ref[m][1][rows, :7])
    Y = X.copy().astype(np.float64)
    Y.data[:] = np.random.RandomState(0).choice([0.5, 2.0, 5.0], len(Y.data))          # any nonzero value counts as 1
    assert np.array_equal(neighbours.cooccur_topk_host(Y, 7, 'cosine')[0], ref['cosine'][0][:, :7])
    # the exact fallback: a float pre-sort that is wrong on purpose must be repaired by the adjacent-pair check
    cmp = neighbours._beats_py('cosine', 9)
    assert cmp((3, 4, 1), (3, 5, 0)) == -1 and cmp((2, 4, 7), (4, 16, 3)) == 1 and cmp((2, 4, 3), (4, 16, 7)) == -1 and cmp((2, 4, 3), (2, 4, 3)) == 0
    with pytest.raises(ValueError):
        neighbours.cooccur_topk_host(X, 0)
    with pytest.raises(ValueError):
        neighbours.cooccur_topk_host(X, 3, 'pearson')
    with pytest.raises(ValueError):
        neighbours.cooccur_topk_host(X, 3, 'cosine', rows=[70])


def test_route_host_of_the_wrapper_canonicalises_its_input(problems):
    """route='host' needs no GPU: unsorted columns and repeats give the result of the canonical matrix, as CPU tensors."""
    import torch
    from arlib_amd import neighbours
    X, ref = problems['random']
    rng = np.random.RandomState(1)
    rp, ci = [0], []
    for u in range(X.shape[0]):
        c = X.indices[X.indptr[u]:X.indptr[u + 1]]
        c = np.concatenate([c, c[:2]])                      # repeats
        ci += rng.permutation(c).tolist()
        rp.append(len(ci))
    idx, cnt, deg = neighbours.cooccur_topk(np.array(rp), np.array(ci), X.shape[0], X.shape[1], 5, 'jaccard', route='host')
    assert isinstance(idx, torch.Tensor) and idx.device.type == 'cpu' and idx.dtype == torch.int32 and deg.dtype == torch.int64
    assert np.array_equal(idx.numpy(), ref['jaccard'][0][:, :5]) and np.array_equal(cnt.numpy(), ref['jaccard'][1][:, :5])
    assert np.array_equal(deg.numpy(), ref['jaccard'][2])


def test_wrapper_raises_value_errors():
    from arlib_amd import neighbours
    rp, ci = np.array([0, 2, 3], np.int64), np.array([0, 1, 1], np.int32)
    ok = dict(rowptr=rp, col=ci, n_rows=2, n_cols=2, k=1, route='host')
    assert neighbours.cooccur_topk(**ok)[0].tolist() == [[1], [0]]
    for bad in (dict(k=0), dict(measure='pearson'), dict(route='fast'), dict(n_rows=3), dict(n_rows=-1), dict(n_cols=1), dict(rowptr=np.array([0, 3, 2])),
                dict(rowptr=np.array([1, 2, 3])), dict(col=np.array([0, -1, 1])), dict(rows=[2]), dict(rows=[-1]), dict(rows=[0.5]), dict(tile_rows=0),
                dict(tile_rows=neighbours.COOCCUR_MAX_TILE_ROWS + 1), dict(col=np.zeros((3, 1), np.int32))):
        with pytest.raises(ValueError):
            neighbours.cooccur_topk(**dict(ok, **bad))
    # the kernel's limits: k and the degree bound of the cosine keys
    assert neighbours.cooccur_supported(128, 'cosine', 2 ** 20) and not neighbours.cooccur_supported(129, 'cosine', 5)
    assert not neighbours.cooccur_supported(5, 'cosine', 2 ** 20 + 1) and neighbours.cooccur_supported(5, 'jaccard', 2 ** 20 + 1)
    with pytest.raises(ValueError, match='cooccur_topk_host'):
        neighbours.cooccur_topk(rp, ci, 2, 2, 129, route='kernel', device='cpu')          # no GPU named: refused before anything is moved


def test_c_entry_refuses_each_defect_before_any_launch():
    from arlib_amd import _lib, neighbours
    L = _lib.lib()
    assert _lib.ABI_VERSION == 34 and L.arl_abi_version() == 34
    assert L.arl_cooccur_max_k() == neighbours.COOCCUR_MAX_K == 128
    assert L.arl_cooccur_max_tile_rows() == neighbours.COOCCUR_MAX_TILE_ROWS and L.arl_cooccur_default_tile_rows() == neighbours.COOCCUR_DEFAULT_TILE_ROWS
    assert 15936 + 4 * neighbours.COOCCUR_MAX_TILE_ROWS <= 160 * 1024 and 15936 + 4 * neighbours.COOCCUR_DEFAULT_TILE_ROWS <= 80 * 1024
    for m, code in neighbours.MEASURES.items():
        assert L.arl_cooccur_max_degree(code) == neighbours.COOCCUR_MAX_DEGREE[m]
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # rowptr col colptr irow n_rows n_cols rows n_queries k measure max_degree order tile_rows idx cnt stream
    good = [p, p, p, p, 4, 4, None, 4, 2, 1, 3, None, 0, p, p, None]

    def call(**kw):
        a = list(good)
        for pos, v in kw.items():
            a[int(pos[1:])] = v
        return L.arl_cooccur_topk_i32(*a)
    NULL, RANGE, ARG = -1, -3, -4
    assert call(_0=None) == NULL and call(_2=None) == NULL and call(_13=None) == NULL and call(_14=None) == NULL
    assert call(_4=-1) == ARG and call(_5=-1) == ARG and call(_7=-1) == ARG and call(_8=0) == ARG and call(_8=-3) == ARG
    assert call(_9=3) == ARG and call(_9=-1) == ARG and call(_10=-1) == ARG and call(_12=-1) == ARG
    assert call(_8=129) == RANGE and call(_12=neighbours.COOCCUR_MAX_TILE_ROWS + 1) == RANGE
    assert call(_4=2 ** 31) == RANGE and call(_5=2 ** 31) == RANGE and call(_7=2 ** 31) == RANGE and call(_7=2 ** 30, _8=2) == RANGE
    assert call(_10=2 ** 20 + 1) == RANGE                   # cosine keys: c^2 d must stay below 2^63
    assert call(_9=0, _10=2 ** 31) == RANGE and call(_9=2, _10=2 ** 31) == RANGE
    assert call(_7=0, _0=None, _2=None, _13=None, _14=None) == 0                                # no queries: nothing to do


def test_detection_metric_hand_computed():
    from arlib_amd.util.metrics import DetectionMetric
    #          id 0    1    2    3    4    5
    scores = [0.9, 0.2, 0.5, 0.5, 0.1, 0.5]
    m = DetectionMetric(scores, [0, 3])
    # pairs (fake, real): 0 beats 1, 2, 4, 5 -> 4; 3 beats 1, 4 and ties 2, 5 -> 2 + 2 * 0.5 = 3; 7 of 8
    assert m.auc() == 7 / 8
    # ranking: 0 (0.9), then the 0.5 tie by id 2, 3, 5, then 1, 4
    assert m.precision_at(1) == 1.0 and m.precision_at(2) == 0.5 and m.precision_at(3) == 2 / 3 and m.precision_at(6) == 2 / 6
    assert m.recall_at(1) == 0.5 and m.recall_at(2) == 0.5 and m.recall_at(3) == 1.0
    assert m.f1_at(2) == 0.5 and m.f1_at(3) == 2 * (2 / 3) * 1.0 / (2 / 3 + 1.0)
    assert m.precision_at(10) == 2 / 6                      # n past the number of users: all of them
    assert DetectionMetric([3.0, 2.0, 1.0, 0.0], [0, 1]).auc() == 1.0 and DetectionMetric([3.0, 2.0, 1.0, 0.0], [2, 3]).auc() == 0.0
    assert DetectionMetric([1.0, 1.0, 1.0], [1]).auc() == 0.5 and DetectionMetric([1.0, 0.0], [0]).f1_at(1) == 1.0
    assert DetectionMetric([1.0, 0.0], [1]).f1_at(1) == 0.0 and np.isnan(DetectionMetric([1.0, 0.0], []).auc())
    for bad in (dict(scores=[1.0, float('nan')], fake_ids=[0]), dict(scores=[1.0, 2.0], fake_ids=[2]), dict(scores=[1.0, 2.0], fake_ids=[0, 0])):
        with pytest.raises(ValueError):
            DetectionMetric(**bad)
    with pytest.raises(ValueError):
        m.precision_at(0)


def test_profile_features_agree_with_direct_numpy():
    from arlib_amd import detect
    X, fake = R.planted()
    D = np.asarray(X.todense(), dtype=np.float64)
    U = D.shape[0]
    k = 10
    f = detect.profile_features(X, k=k, measure='cosine')
    assert set(f) == {'degsim', 'knn_indegree', 'length_var', 'mean_popularity'} and all(v.dtype == np.float64 and v.shape == (U,) for v in f.values())
    n = D.sum(1)
    C = D @ D.T
    S = C / np.sqrt(np.outer(n, n))
    np.fill_diagonal(S, -1.0)
    top = -np.sort(-S, 1)[:, :k]
    assert np.abs(f['degsim'] - np.maximum(top, 0.0).sum(1) / k).max() < 1e-12
    ridx, rcnt, rdeg = R.cooccur_topk(X, k, 'cosine')
    assert np.array_equal(f['degsim'], R.similarity(ridx, rcnt, rdeg, None, 'cosine').sum(1) / k)
    assert np.array_equal(f['knn_indegree'], np.bincount(ridx[ridx >= 0], minlength=U).astype(np.float64))
    assert np.allclose(f['length_var'], np.abs(n - n.mean()) / ((n - n.mean()) ** 2).sum(), rtol=1e-13, atol=0)
    pop = D.sum(0) / U
    assert np.allclose(f['mean_popularity'], (D * pop).sum(1) / n, rtol=1e-13, atol=0)
    # the detector and sanitize on top of it
    det = detect.DegSimDetector(k=k, measure='cosine')
    assert np.array_equal(det.score(X), f['degsim'])
    assert sorted(det.flag(X, len(fake)).tolist()) == fake.tolist()
    kept, reduced = detect.sanitize(X, f['degsim'], len(fake))
    assert kept.tolist() == list(range(U - len(fake))) and reduced.shape == (U - len(fake), X.shape[1]) and (reduced != X[:U - len(fake)]).nnz == 0
    assert detect.sanitize(X, f['degsim'], 0)[0].tolist() == list(range(U))
    with pytest.raises(ValueError):
        detect.sanitize(X, f['degsim'][:-1], 1)
    # degenerate inputs: equal lengths, an empty profile
    g = detect.profile_features(sp.csr_matrix(np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1]])), k=2, measure='jaccard')
    assert g['length_var'].tolist() == [0.0, 0.0, 0.0] and g['degsim'].tolist() == [1 / 3, 1 / 3, 1 / 3] and g['knn_indegree'].tolist() == [2.0, 2.0, 2.0]
    h = detect.profile_features(sp.csr_matrix(np.array([[1, 1], [0, 0], [1, 0]])), k=1, measure='count')
    assert h['degsim'].tolist() == [1.0, 0.0, 1.0] and h['mean_popularity'].tolist() == [0.5, 0.0, 2 / 3] and h['knn_indegree'].tolist() == [1.0, 0.0, 1.0]


def test_host_route_past_the_int64_bound_sorts_with_python_ints():
    """A row of 2^20 + 5 columns: c^2 d no longer fits 64 bits for cosine, the kernel is not offered and the host route orders with Python ints."""
    from arlib_amd import neighbours
    n_cols = 2 ** 20 + 5
    r = np.concatenate([np.zeros(n_cols, np.int64), np.array([1, 1, 1, 2, 2, 3, 3, 3, 3, 4])])
    c = np.concatenate([np.arange(n_cols), np.array([0, 1, 2, 0, 7, 3, 4, 5, 6, 1])])
    X = sp.csr_matrix((np.ones(len(r), np.int64), (r, c)), shape=(5, n_cols))
    assert not neighbours.cooccur_supported(3, 'cosine', n_cols) and neighbours.cooccur_supported(3, 'jaccard', n_cols)
    for measure in MEASURES:
        got, ref = neighbours.cooccur_topk_host(X, 3, measure), R.cooccur_topk(X, 3, measure)
        assert all(np.array_equal(g, x) for g, x in zip(got, ref)), measure
    # cosine from row 0: c^2 / d = 9/3, 4/2, 16/4, 1/1 -> 3 (16/4), 1 (9/3), 2 (4/2)
    assert neighbours.cooccur_topk_host(X, 3, 'cosine')[0][0].tolist() == [3, 1, 2]
    idx, cnt, deg = neighbours.cooccur_topk(X.indptr, X.indices, 5, n_cols, 3, 'cosine', route='auto', device='cpu')      # past the limit: the host route
    assert idx[0].tolist() == [3, 1, 2] and cnt[0].tolist() == [4, 3, 2] and int(deg[0]) == n_cols


def test_without_a_gpu_device_auto_takes_the_host_route_and_kernel_raises(problems, monkeypatch):
    """A problem inside the kernel's limits on device='cpu': the C entry must never see host memory."""
    import torch
    from arlib_amd import _lib, neighbours
    X, ref = problems['random']
    assert neighbours.cooccur_supported(5, 'cosine', int(np.diff(X.indptr).max()), *X.shape, X.shape[0])
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was reached'))
    for rp, ci in ((X.indptr, X.indices), (torch.from_numpy(X.indptr.astype(np.int64)), torch.from_numpy(X.indices.astype(np.int32)))):
        idx, cnt, deg = neighbours.cooccur_topk(rp, ci, X.shape[0], X.shape[1], 5, 'cosine', device='cpu', route='auto')
        assert idx.device.type == 'cpu' and np.array_equal(idx.numpy(), ref['cosine'][0][:, :5]) and np.array_equal(cnt.numpy(), ref['cosine'][1][:, :5])
        with pytest.raises(ValueError, match='needs a GPU'):
            neighbours.cooccur_topk(rp, ci, X.shape[0], X.shape[1], 5, 'cosine', device='cpu', route='kernel')
    # ids are checked at their own width, rows must be integers
    with pytest.raises(ValueError, match='column id'):
        neighbours.cooccur_topk(np.array([0, 1]), np.array([2 ** 32 + 1], np.int64), 1, 4, 1, route='host')
    for bad in (dict(col=np.array([0.0, 1.0, 1.0])), dict(rows=np.array([True, False]))):
        with pytest.raises(ValueError):
            neighbours.cooccur_topk(**dict(dict(rowptr=np.array([0, 2, 3]), col=np.array([0, 1, 1]), n_rows=2, n_cols=2, k=1, route='host'), **bad))

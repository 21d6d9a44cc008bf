"""Device k-means (arlib_amd/cluster.py, csrc/arl_kmeans.hip) against float64 restatements written here in numpy: the assign pass at ragged sizes,
its tie / NaN rules, the update pass (empty cluster, a segment longer than a chunk), the whole Lloyd loop, run-to-run bits, and NCL's opt-in
`kmeans = 'device'` back end on the ml-100k fixture."""
import contextlib
import io
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from test_host_api import make_data

pytestmark = pytest.mark.gpu
DEV = 'cuda'
U32 = 2.0 ** -24                                    # fp32 unit round-off


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- float64 restatements
def scores64(X, C):
    X, C = X.astype(np.float64), C.astype(np.float64)
    return X @ C.T - 0.5 * (C * C).sum(1)[None, :]


def score_bound(X, C):
    """4 d 2^-24 (|x| max|c| + 1/2 max|c|^2) per row: the fp32 dot-product bound on two scores plus bias."""
    X, C = X.astype(np.float64), C.astype(np.float64)
    cn = np.sqrt((C * C).sum(1)).max()
    return 4.0 * X.shape[1] * U32 * (np.sqrt((X * X).sum(1)) * cn + 0.5 * cn * cn)


def check_assign(X, C, labels, score=None):
    """A label may differ from float64's only where float64's gap between its best and second-best score is within score_bound; at most 1 % of
    the rows may be excused that way; the returned score is within the bound of the float64 score of the chosen centroid.  Returns the number excused."""
    N, k = X.shape[0], C.shape[0]
    S, bound = scores64(X, C), score_bound(X, C)
    labels = np.asarray(labels).astype(np.int64)
    assert labels.shape == (N,) and labels.min() >= 0 and labels.max() < k
    best = S.argmax(1)
    if k > 1:
        top2 = np.partition(S, k - 2, axis=1)[:, k - 2:]
        gap = top2[:, 1] - top2[:, 0]
    else:
        gap = np.full(N, np.inf)
    differ = labels != best
    assert not (differ & ~(gap <= bound)).any(), 'labels differ from float64 where its gap is above the bound: rows %s' % np.nonzero(differ & ~(gap <= bound))[0][:10]
    print('assign N=%d k=%d d=%d: %d labels differ (all excused), tightest gap/bound %.3g' % (N, k, X.shape[1], differ.sum(), (gap / bound).min()))
    assert differ.sum() <= N // 100
    if score is not None:
        err = np.abs(np.asarray(score).astype(np.float64) - S[np.arange(N), labels])
        print('    score error / bound: max %.3g' % (err / bound).max())
        assert (err <= bound).all()
    return int(differ.sum())


def means64(X, labels, C_prev):
    X64, k = X.astype(np.float64), C_prev.shape[0]
    counts = np.bincount(labels, minlength=k)
    C = C_prev.astype(np.float64).copy()
    for c in np.nonzero(counts)[0]:
        C[c] = X64[labels == c].mean(0)
    return C, counts


def mean_bound(X, labels, k):
    """n_c 2^-24 max|x| over the members, per component: the sequential-sum worst case (any summation order stays inside it)."""
    B = np.zeros((k, X.shape[1]))
    for c in np.unique(labels):
        m = labels == c
        B[c] = m.sum() * U32 * np.abs(X[m].astype(np.float64)).max(0)
    return B


def lloyd64(X, init, n_iter):
    """The loop of cluster.kmeans in float64: ties to the lower index (argmax), an empty cluster keeps its centroid."""
    X64, C = X.astype(np.float64), init.astype(np.float64).copy()
    inertia, prev, done, gaps = [], None, 0, []
    while True:
        S = scores64(X64, C)
        labels = S.argmax(1)
        top2 = np.partition(S, S.shape[1] - 2, axis=1)[:, -2:]
        gaps.append(((top2[:, 1] - top2[:, 0]) / score_bound(X64, C)).min())
        inertia.append(((X64 - C[labels]) ** 2).sum())
        if (prev is not None and (labels == prev).all()) or done == n_iter:
            break
        C, _ = means64(X64, labels, C)
        prev, done = labels, done + 1
    return C, labels, inertia, done, min(gaps)


# ---------------------------------------------------------------------------------------------------------------- 1. assign
@pytest.mark.parametrize('N,k,d', [(1061, 200, 64), (1061, 65, 16), (1061, 63, 32), (1061, 200, 128), (4133, 2000, 64), (17, 1, 64), (1, 1, 16)])
def test_assign_against_float64(N, k, d):
    from arlib_amd import cluster
    rng = np.random.default_rng(N + k + d)
    X, C = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((k, d)).astype(np.float32)
    labels, score = cluster.kmeans_assign(dev(X), dev(C))
    assert labels.dtype == torch.int32 and score.dtype == torch.float32 and labels.shape == (N,) and score.shape == (N,)
    check_assign(X, C, labels.cpu().numpy(), score.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- 2. ties and safety
def test_ties_go_to_the_lower_index():
    from arlib_amd import cluster
    rng = np.random.default_rng(5)
    X, C = rng.standard_normal((1061, 64)).astype(np.float32), rng.standard_normal((200, 64)).astype(np.float32)
    X[:300] = C[5] + 0.05 * rng.standard_normal((300, 64)).astype(np.float32)          # rows that do choose the duplicated centroid
    for dup in (9, 6, 70, 199):                  # another lane group of the same tile, the same lane, a later stage, the ragged last stage
        C[dup] = C[5]
    labels = cluster.kmeans_assign(dev(X), dev(C))[0].cpu().numpy()
    assert (labels[:300] == 5).all()
    assert not np.isin(labels, (9, 6, 70, 199)).any()
    check_assign(X, np.delete(C, (6, 9, 70, 199), 0), labels - (labels > 6) - (labels > 9) - (labels > 70))


@pytest.mark.parametrize('N,k,d', [(1061, 200, 64), (130, 7, 16)])
def test_all_equal_rows_and_centroids_give_label_zero(N, k, d):
    from arlib_amd import cluster
    row = np.random.default_rng(1).standard_normal(d).astype(np.float32)
    labels, score = cluster.kmeans_assign(dev(np.tile(row, (N, 1))), dev(np.tile(row, (k, 1))))
    assert int(labels.abs().max()) == 0
    assert len(set(score.cpu().numpy().tolist())) == 1


def test_nan_row_stays_in_range_and_alone():
    from arlib_amd import cluster
    rng = np.random.default_rng(2)
    X, C = rng.standard_normal((1061, 64)).astype(np.float32), rng.standard_normal((200, 64)).astype(np.float32)
    clean = cluster.kmeans_assign(dev(X), dev(C))[0].cpu().numpy()
    X[517] = np.nan
    labels = cluster.kmeans_assign(dev(X), dev(C))[0].cpu().numpy()
    assert labels.min() >= 0 and labels.max() < 200 and labels[517] == 0
    keep = np.arange(1061) != 517
    assert np.array_equal(labels[keep], clean[keep])
    # and through the loop: the update takes the labels as they are, nothing indexes out of range
    Cn, lab, _, _ = cluster.kmeans(dev(X), 200, n_iter=2, init=dev(C))
    assert int(lab.min()) >= 0 and int(lab.max()) < 200 and Cn.shape == (200, 64)


# ---------------------------------------------------------------------------------------------------------------- 3. update
def update_case(N, k, d, big, big_n, empty, seed):
    rng = np.random.default_rng(seed)
    X, C_prev = rng.standard_normal((N, d)).astype(np.float32), rng.standard_normal((k, d)).astype(np.float32)
    others = np.array([c for c in range(k) if c not in (empty, big)])
    labels = others[rng.integers(0, len(others), N)]
    labels[rng.permutation(N)[:big_n]] = big
    return X, labels.astype(np.int64), C_prev


@pytest.mark.parametrize('N,k,d,big,big_n,empty', [(1061, 200, 64, 3, 600, 7), (20011, 3, 64, 1, 19000, 2), (20011, 3, 16, 0, 19000, 1), (1061, 200, 128, 3, 600, 7),
                                                   (777, 5, 32, 4, 300, 0)])
@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_update_against_float64_means(N, k, d, big, big_n, empty, dtype):
    from arlib_amd import cluster, _lib
    assert big_n > _lib.lib().arl_kmeans_chunk_rows()                       # the large cluster spans several chunks
    X, labels, C_prev = update_case(N, k, d, big, big_n, empty, seed=N + d)
    C_new, counts = cluster.kmeans_update(dev(X), dev(labels).to(dtype), dev(C_prev))
    want, want_counts = means64(X, labels, C_prev)
    assert want_counts[empty] == 0 and want_counts[big] >= big_n
    assert counts.dtype == torch.int64 and np.array_equal(counts.cpu().numpy(), want_counts)
    got = C_new.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (k, d)
    assert np.array_equal(got[empty].view(np.uint32), C_prev[empty].view(np.uint32))
    B = mean_bound(X, labels, k)
    filled = want_counts > 0
    err = np.abs(got.astype(np.float64) - want)
    print('update N=%d k=%d d=%d: error / bound max %.3g' % (N, k, d, (err[filled] / B[filled]).max()))
    assert (err[filled] <= B[filled]).all()


def test_update_rejects_labels_out_of_range():
    from arlib_amd import cluster
    X, labels, C_prev = update_case(300, 5, 16, 1, 260, 2, seed=0)
    for bad in (-1, 5):
        l = labels.copy(); l[17] = bad
        with pytest.raises(ValueError):
            cluster.kmeans_update(dev(X), dev(l), dev(C_prev))
    with pytest.raises(ValueError):
        cluster.kmeans(dev(X), 5, init=dev(C_prev[:4]))


def test_device_tensors_of_a_bad_width_or_dtype_are_refused():
    from arlib_amd import cluster
    for width in (24, 256):
        bad = torch.zeros(300, width, device=DEV)
        with pytest.raises(ValueError, match='width %d outside' % width):
            cluster.kmeans(bad, 5)
        with pytest.raises(ValueError, match='width %d outside' % width):
            cluster.kmeans_assign(bad, bad[:5])
    for dtype in (torch.float64, torch.float16):
        bad = torch.zeros(300, 64, device=DEV, dtype=dtype)
        with pytest.raises(ValueError, match='must be float32'):
            cluster.kmeans(bad, 5)
        with pytest.raises(ValueError, match='must be float32'):
            cluster.kmeans_update(torch.zeros(300, 64, device=DEV), torch.zeros(300, dtype=torch.int64, device=DEV), bad[:5])
    with pytest.raises(ValueError, match='on one device'):
        cluster.kmeans_assign(torch.zeros(300, 64, device=DEV), torch.zeros(5, 32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- 4. Lloyd
def blobs(d, seed, spread, N=2000, k=10):
    """Ten separated blobs (centres 2 N(0, 1) per component, points 0.5 N(0, 1) around them) and a start of the centres moved by spread N(0, 1):
    far enough that the first assign passes are wrong for some blobs, the labels move for a few passes and a centroid may end without members."""
    rng = np.random.default_rng(seed)
    centres = 2.0 * rng.standard_normal((k, d))
    X = (centres[rng.integers(0, k, N)] + 0.5 * rng.standard_normal((N, d))).astype(np.float32)
    init = (centres + spread * rng.standard_normal((k, d))).astype(np.float32)
    return X, init


@pytest.mark.parametrize('d,seed,spread', [(16, 3, 2.5), (64, 3, 5.0)])
def test_lloyd_against_float64_lloyd(d, seed, spread):
    from arlib_amd import cluster
    X, init = blobs(d, seed, spread)
    want_C, want_labels, want_inertia, want_iters, tightest = lloyd64(X, init, 50)
    # the data: float64 never decides inside the fp32 bound (so the labels of every pass are determined), several passes move labels, one cluster ends empty
    assert tightest > 2.0 and 2 <= want_iters < 50 and np.bincount(want_labels, minlength=10).min() == 0
    C, labels, inertia, iters = cluster.kmeans(dev(X), 10, n_iter=50, init=dev(init))
    assert C.dtype == torch.float32 and C.shape == (10, d) and labels.dtype == torch.int64 and labels.shape == (2000,) and C.is_cuda and labels.is_cuda
    assert iters == want_iters and len(inertia) == iters + 1
    labels = labels.cpu().numpy()
    assert np.array_equal(labels, want_labels)
    err, B = np.abs(C.cpu().numpy().astype(np.float64) - want_C), mean_bound(X, labels, 10)
    filled = np.bincount(labels, minlength=10) > 0
    assert (err[filled] <= B[filled]).all()
    assert (err[~filled] <= 2000 * U32 * np.abs(X).max()).all()             # kept from the pass that last filled it: the bound of a cluster of all rows
    tol = 8.0 * d * U32
    print('lloyd d=%d: %d updates, inertia %s, float64 last %.9g' % (d, iters, ['%.9g' % v for v in inertia], want_inertia[-1]))
    assert all(b <= a * (1.0 + tol) for a, b in zip(inertia, inertia[1:]))
    assert abs(inertia[-1] - want_inertia[-1]) <= tol * want_inertia[-1]
    # n_iter bounds the updates; the labels still belong to the centroids returned
    C2, labels2, inertia2, iters2 = cluster.kmeans(dev(X), 10, n_iter=1, init=dev(init))
    assert iters2 == 1 and len(inertia2) == 2
    check_assign(X, C2.cpu().numpy(), labels2.cpu().numpy())


# ---------------------------------------------------------------------------------------------------------------- 5. determinism
def test_two_runs_give_the_same_bits():
    from arlib_amd import cluster
    X, init = blobs(64, 3, 5.0)
    Xd = dev(X)
    a, b = cluster.kmeans(Xd, 10, init=dev(init)), cluster.kmeans(Xd, 10, init=dev(init))
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    np.random.seed(11)
    a = cluster.kmeans(Xd, 10)
    np.random.seed(11)
    want_init = X[np.random.choice(2000, 10, replace=False)]
    np.random.seed(11)
    b = cluster.kmeans(Xd, 10)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]
    c = cluster.kmeans(Xd, 10, init=dev(want_init))                         # init=None is that draw and nothing else
    assert torch.equal(a[0].view(torch.int32), c[0].view(torch.int32)) and torch.equal(a[1], c[1]) and a[2] == c[2]


# ---------------------------------------------------------------------------------------------------------------- 6. NCL
def rec_args(**kw):
    a = dict(dataset='ml-100k', model_name='NCL', maxEpoch=30, batch_size=2048, emb_size=16, n_layers=2, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


def _raiser(what):
    def raising(*a, **k):
        raise AssertionError(what + ' was called')
    return raising


def test_ncl_device_backend(tmp_path, monkeypatch):
    import sklearn.cluster
    from arlib_amd.recommender.NCL import NCL
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(sklearn.cluster, 'KMeans', _raiser('sklearn.cluster.KMeans'))
    data = make_data()
    with contextlib.redirect_stdout(io.StringIO()):
        rec = NCL(rec_args(ncl_kmeans='device'), data)
    assert rec.kmeans == 'device'
    rec.k = 50
    model = rec.model.cuda()
    np.random.seed(515)
    rec.e_step()
    for table, cent, lab in ((model.embedding_dict['user_emb'], rec.user_centroids, rec.user_2cluster),
                             (model.embedding_dict['item_emb'], rec.item_centroids, rec.item_2cluster)):
        N, d = table.shape
        assert cent.dtype == torch.float32 and cent.shape == (50, d) and cent.device == table.device
        assert lab.dtype == torch.int64 and lab.shape == (N,) and lab.device == table.device
        check_assign(table.detach().cpu().numpy(), cent.cpu().numpy(), lab.cpu().numpy())
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train(Epoch=7, evalNum=5)                                       # epochs 5 and 6 run the prototype phase
    assert rec._epoch == 6 and rec.user_centroids.shape == (50, 16)
    assert np.isfinite(rec.user_emb.cpu().numpy()).all() and np.isfinite(rec.item_emb.cpu().numpy()).all()


def test_ncl_default_backend_calls_sklearn_only(monkeypatch):
    import sklearn.cluster
    from arlib_amd import cluster
    from arlib_amd.recommender.NCL import NCL
    calls, real = [], sklearn.cluster.KMeans

    def recording(*a, **k):
        calls.append(k)
        return real(*a, **k)
    monkeypatch.setattr(sklearn.cluster, 'KMeans', recording)
    monkeypatch.setattr(cluster, 'kmeans', _raiser('cluster.kmeans'))
    data = make_data()
    with contextlib.redirect_stdout(io.StringIO()):
        rec = NCL(rec_args(), data)
    assert rec.kmeans == 'sklearn'
    rec.k = 50
    rec.model.cuda()
    np.random.seed(515)
    rec.e_step()
    assert calls == [{'n_clusters': 50}, {'n_clusters': 50}]
    assert rec.user_centroids.shape == (50, 16) and rec.user_2cluster.dtype == torch.int64 and rec.user_2cluster.is_cuda

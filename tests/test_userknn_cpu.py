"""arlib_amd.userknn, recommender.UserKNN and the metric hooks without a GPU: the host route against the pure-Python restatement
(tests/userknn_restatement.py), weight_matrix and neighbour_share against hand values, UserKNN end to end on the host routes, AttackMetric and
TargetRankMetric on it, the wrapper's ValueErrors and the C entry's ARL_E_* codes (the library loads without a device and refuses before any
launch).  Every comparison is array_equal: the results are integers."""
import contextlib
import ctypes
import io
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import userknn_restatement as R

TARGETS = {1: [391], 5: [390, 391, 392, 0, 6]}
TARGETS[64] = [390, 391, 392] + [i for i in range(0, 400, 6) if i not in (390, 391, 392)][:61]


@pytest.fixture(scope='module')
def planted():
    """The planted 320 x 400 input, its restated user-side lists (k = 7, cosine) and the restated result at N = 128 with and without the mask
    and with the 64 targets: computed once, read by every test."""
    X, _ = R.planted()
    ni, nw = R.lists_of(X, 7, 'cosine')
    ref = {m: R.uknn_score_topk(X, ni, nw, 128, mask_profile=m, targets=TARGETS[64]) for m in (False, True)}
    return X, ni, nw, ref


@pytest.mark.parametrize('mask', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('N', [1, 10, 128])
def test_host_route_equals_the_restatement(planted, N, mask):
    from arlib_amd import userknn
    X, ni, nw, ref = planted
    assert X.shape == (320, 400) and ni.shape == (320, 7)
    idx, score, rank = userknn.uknn_score_topk_host(X, ni, nw, N, mask_profile=mask, targets=TARGETS[64])
    assert idx.dtype == np.int32 and score.dtype == np.int64 and rank.dtype == np.int32 and idx.shape == (320, N) and rank.shape == (320, 64)
    assert np.array_equal(idx, ref[mask][0][:, :N]) and np.array_equal(score, ref[mask][1][:, :N]) and np.array_equal(rank, ref[mask][2])
    assert userknn.uknn_score_topk_host(X, ni, nw, N, mask_profile=mask)[2] is None
    # the fake rows hold the targets 390..392: masked there, ranked everywhere when nothing is masked
    assert (rank[300:, :3] == -1).all() == mask and ((rank >= 0).all() != mask)
    # small chunks give the same result
    small = userknn.uknn_score_topk_host(X, ni, nw, N, mask_profile=mask, targets=TARGETS[64], chunk_rows=37)
    assert all(np.array_equal(a, b) for a, b in zip(small, (idx, score, rank)))


@pytest.mark.parametrize('T', [1, 5, 64])
def test_host_route_rows_subset_with_a_repeat_and_targets(planted, T):
    from arlib_amd import userknn
    X, ni, nw, ref = planted
    rows = np.random.RandomState(5).permutation(320)[:41]
    rows[30] = rows[3]
    rows[7] = 305                                           # a fake row: its targets are masked
    col = [TARGETS[64].index(t) for t in TARGETS[T]]
    for mask in (False, True):
        idx, score, rank = userknn.uknn_score_topk_host(X, ni, nw, 10, rows, mask, TARGETS[T])
        assert np.array_equal(idx, ref[mask][0][rows, :10]) and np.array_equal(score, ref[mask][1][rows, :10])
        assert np.array_equal(rank, ref[mask][2][rows][:, col])
    assert (rank[7, :1] == -1).all() and rank.shape == (41, T)
    # the wrapper's host route canonicalises its input and returns CPU tensors
    rp, ci = X.indptr.astype(np.int64), X.indices.astype(np.int32)
    wi, ws, wr = userknn.uknn_score_topk(rp, ci, 320, 400, ni, nw, 10, rows=rows, mask_profile=True, targets=TARGETS[T], route='host')
    assert isinstance(wi, torch.Tensor) and wi.dtype == torch.int32 and ws.dtype == torch.int64 and wr.dtype == torch.int32
    assert np.array_equal(wi.numpy(), idx) and np.array_equal(ws.numpy(), score) and np.array_equal(wr.numpy(), rank)


def test_unsorted_and_repeated_entries_equal_the_canonical_input(planted):
    from arlib_amd import userknn
    X, ni, nw, ref = planted
    rng = np.random.RandomState(8)
    rp, ci = [0], []
    for u in range(X.shape[0]):
        c = X.indices[X.indptr[u]:X.indptr[u + 1]]
        ci += rng.permutation(np.concatenate([c, c[:3], c[-1:]])).tolist()
        rp.append(len(ci))
    idx, score, rank = userknn.uknn_score_topk(np.array(rp), np.array(ci), 320, 400, ni, nw, 16, mask_profile=True, targets=TARGETS[64], device='cpu')
    assert np.array_equal(idx.numpy(), ref[True][0][:, :16]) and np.array_equal(score.numpy(), ref[True][1][:, :16]) and np.array_equal(rank.numpy(), ref[True][2])


def test_the_sum_is_taken_as_written():
    """A slot naming u itself, a neighbour in two slots and -1 in the middle of a list, by hand and against the restatement."""
    from arlib_amd import userknn
    #   user 0: {0, 1}   user 1: {1, 2}   user 2: {3}
    X = sp.csr_matrix(np.array([[1, 1, 0, 0, 0], [0, 1, 1, 0, 0], [0, 0, 0, 1, 0]], np.int64))
    ni = np.array([[0, -1, 1], [2, 2, -1], [-1, -1, -1]], np.int32)
    nw = np.array([[4, 99, 3], [5, 6, 77], [1, 2, 3]], np.int32)
    idx, score, rank = userknn.uknn_score_topk_host(X, ni, nw, 5, targets=[3, 1, 4])
    # user 0: itself with 4 on {0, 1}, user 1 with 3 on {1, 2}: scores 4, 7, 3, 0, 0.  user 1: user 2 twice: 11 on item 3.  user 2: nothing
    assert idx.tolist() == [[1, 0, 2, 3, 4], [3, 0, 1, 2, 4], [0, 1, 2, 3, 4]]
    assert score.tolist() == [[7, 4, 3, 0, 0], [11, 0, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert rank.tolist() == [[3, 0, 4], [0, 2, 4], [3, 1, 4]]
    ref = R.uknn_score_topk(X, ni, nw, 5, targets=[3, 1, 4])
    assert np.array_equal(idx, ref[0]) and np.array_equal(score, ref[1]) and np.array_equal(rank, ref[2])
    idx, score, rank = userknn.uknn_score_topk_host(X, ni, nw, 5, mask_profile=True, targets=[3, 1, 4])
    assert idx.tolist() == [[2, 3, 4, -1, -1], [3, 0, 4, -1, -1], [0, 1, 2, 4, -1]] and score[0].tolist() == [3, 0, 0, 0, 0]
    assert rank.tolist() == [[1, -1, 2], [0, -1, 2], [-1, 1, 3]]
    ref = R.uknn_score_topk(X, ni, nw, 5, mask_profile=True, targets=[3, 1, 4])
    assert np.array_equal(idx, ref[0]) and np.array_equal(score, ref[1]) and np.array_equal(rank, ref[2])


def test_weight_matrix_hand_values():
    from arlib_amd import userknn
    ni = np.array([[0, -1, 1], [2, 2, -1], [-1, -1, -1]], np.int32)
    nw = np.array([[4, 99, 3], [5, 6, 77], [1, 2, 3]], np.int32)
    W = userknn.weight_matrix(ni, nw, 3)
    assert W.shape == (3, 3) and W.dtype == np.int64 and W.toarray().tolist() == [[4, 3, 0], [0, 0, 11], [0, 0, 0]]
    Wq = userknn.weight_matrix(ni, nw, 3, rows=[1, 1, 0])
    assert Wq.shape == (3, 3) and Wq.toarray().tolist() == [[0, 0, 11], [0, 0, 11], [4, 3, 0]]
    big = userknn.weight_matrix(np.array([[1, 1]]), np.array([[2 ** 31 - 1, 2 ** 31 - 1]]), 2)
    assert big.toarray().tolist() == [[0, 2 ** 32 - 2]]      # int64: no wrap


# ------------------------------------------------------------------------------------------------ the model
def synthetic_data(n_users=60, n_items=90, seed=4):
    """A random 60 x 90 DataLoader: of every user with six or more items the last one is held out."""
    from arlib_amd.util.DataLoader import DataLoader
    rng = np.random.RandomState(seed)
    p = (1.0 + np.arange(n_items)) ** -0.7
    p /= p.sum()
    pairs = np.array(sorted((u, int(i)) for u in range(n_users) for i in rng.choice(n_items, rng.randint(3, 16), replace=False, p=p)))
    last = np.r_[pairs[1:, 0] != pairs[:-1, 0], True]
    test = last & (np.bincount(pairs[:, 0], minlength=n_users)[pairs[:, 0]] >= 6)
    tr, te = pairs[~test], pairs[test]
    one = lambda q: (q[:, 0], q[:, 1], np.ones(len(q)))
    return DataLoader.from_arrays(one(tr), None, one(te), dataName='syn', array_native=False)


def rec_args(**kw):
    a = dict(dataset='syn', model_name='UserKNN', maxEpoch=1, batch_size=2048, emb_size=16, n_layers=0, reg=1e-4, lRate=0.01, seed=2018, topK='5,10',
             knn_k=7, knn_route='host')
    a.update(kw)
    return SimpleNamespace(**a)


def trained(data, **kw):
    from arlib_amd.recommender import UserKNN
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rec = UserKNN(rec_args(**kw), data)
        rec.train()
    return rec, buf.getvalue()


@pytest.fixture(scope='module')
def data():
    return synthetic_data()


def model_matrix(data):
    from arlib_amd import neighbours
    return neighbours.binary_csr(data.interaction_mat)


@pytest.mark.parametrize('measure', ['cosine', 'count'])
def test_userknn_end_to_end_on_the_host_route(data, measure):
    from arlib_amd import neighbours
    from arlib_amd.util.metrics import ranking_evaluation
    state = (torch.random.get_rng_state().clone(), np.random.get_state()[1].copy())
    rec, out = trained(data, knn_measure=measure)
    assert 'Recommender: UserKNN' in out and 'Real-Time Ranking Performance' in out
    assert rec.bestPerformance[0] == 1 and set(rec.bestPerformance[1]) == {'Hit Ratio', 'Precision', 'Recall', 'NDCG'}
    assert torch.equal(torch.random.get_rng_state(), state[0]) and np.array_equal(np.random.get_state()[1], state[1])       # nothing was drawn
    X = model_matrix(data)
    assert X.shape == (60, data.item_num) and data.item_num <= 90                      # the items of the 60 x 90 draw that the training part holds
    hi, hc, hd = neighbours.cooccur_topk_host(X, 7, measure)
    assert np.array_equal(rec.nbr_idx, hi) and np.array_equal(rec.nbr_cnt, hc) and np.array_equal(rec.user_deg, hd)
    ni, nw = R.lists_of(X, 7, measure)
    assert np.array_equal(rec.nbr_idx, ni) and np.array_equal(rec.nbr_w, nw)
    users = list(data.test_set)
    rows = [data.user[u] for u in users]
    ridx, rscore, _ = R.uknn_score_topk(X, ni, nw, 10, rows=rows, mask_profile=True)
    with contextlib.redirect_stdout(io.StringIO()):
        rec_list, measure_lines = rec.test()
    assert list(rec_list) == users and len(users) > 20
    scale = 1.0 if measure == 'count' else 2.0 ** 30
    for r, u in enumerate(users):
        assert [it for it, _ in rec_list[u]] == [data.id2item[int(i)] for i in ridx[r]]
        assert [s for _, s in rec_list[u]] == [int(s) / scale for s in rscore[r]]
        assert not set(it for it, _ in rec_list[u]) & set(data.training_set_u[u])
    assert measure_lines == ranking_evaluation(data.test_set, rec_list, [5, 10]) and measure_lines[0] == 'Top 5\n'
    assert rec.bestPerformance[1]['Recall'] == float(measure_lines[-2].strip().split(':')[1])
    # predict: the dense row the lists were cut from; neighbours_of: the list with float similarities
    u = users[3]
    row = rec.predict(u)
    assert row.shape == (data.item_num,) and row.dtype == np.float64
    full, fscore, _ = R.uknn_score_topk(X, ni, nw, data.item_num, rows=[data.user[u]])
    assert np.array_equal(row[full[0]], fscore[0] / scale)
    j = int(np.argmax(rec.user_deg))
    nb = rec.neighbours_of(data.id2user[j])
    assert [v for v, _ in nb] == [data.id2user[int(v)] for v in ni[j] if v >= 0] and len(nb) == 7
    if measure == 'cosine':
        assert all(int(np.floor(s * 2 ** 30)) == int(w) for (_, s), w in zip(nb, nw[j]))
    # the hooks against the restatement
    tg = [3, 40, data.item_num - 1]
    all_rows = [data.user[x] for x in data.user]
    aidx, _, arank = R.uknn_score_topk(X, ni, nw, 12, rows=all_rows, targets=tg)
    assert np.array_equal(rec.topk_all_users(12), aidx) and np.array_equal(rec.target_ranks(tg), arank)
    midx, _, mrank = R.uknn_score_topk(X, ni, nw, 12, rows=all_rows, mask_profile=True, targets=tg)
    assert np.array_equal(rec.topk_all_users(12, mask_train=True), midx) and np.array_equal(rec.target_ranks(tg, mask_train=True), mrank)
    for kw in (dict(requires_grad=True), dict(requires_embgrad=True), dict(requires_adjgrad=True)):
        with pytest.raises(NotImplementedError):
            rec.train(**kw)


def test_model_settings_and_guards(data):
    from arlib_amd import recommender
    from arlib_amd.recommender import ItemKNN, UserKNN
    from arlib_amd.recommender._knn import KNNRecommender
    assert 'UserKNN' in recommender.__all__ and issubclass(UserKNN, KNNRecommender) and issubclass(ItemKNN, KNNRecommender)
    args = rec_args()
    for k in ('knn_k', 'knn_route'):
        delattr(args, k)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = UserKNN(args, data)
        assert (plain.knn_k, plain.knn_measure, plain.knn_shrink, plain.knn_route) == (50, 'cosine', 0.0, 'auto')
        custom = UserKNN(rec_args(knn_k=3, knn_measure='jaccard', knn_shrink=2.5, knn_route='host'), data)
        assert (custom.knn_k, custom.knn_measure, custom.knn_shrink, custom.knn_route) == (3, 'jaccard', 2.5, 'host')
        for bad in (dict(knn_k=0), dict(knn_measure='pearson'), dict(knn_shrink=-1.0), dict(knn_route='fast')):
            with pytest.raises(ValueError):
                UserKNN(rec_args(**bad), data)
        for call in (lambda: plain.predict(data.id2user[0]), lambda: plain.neighbours_of(data.id2user[0]), lambda: plain.neighbour_share([]),
                     lambda: plain.topk_all_users(5)):
            with pytest.raises(RuntimeError, match='UserKNN: train'):
                call()


def test_attack_metrics_on_a_userknn_agree_with_each_other_at_every_k(data):
    from arlib_amd.util.metrics import AttackMetric, TargetRankMetric
    rec, _ = trained(data)
    targets = [3, 40, data.item_num - 1, 17]
    ks = [1, 5, 10, 50, data.item_num]
    a, t = AttackMetric(rec, targets, top=ks), TargetRankMetric(rec, targets, top=ks)
    for name in ('precision', 'hitRate', 'recall'):          # integer counts, divided once
        assert getattr(a, name)() == getattr(t, name)(), name
    # the hit matrix behind every figure, in integers: position r of user u's list holds a target exactly when some target has rank r
    hit, rk = a._hits(), t.ranks()
    from_ranks = np.zeros(hit.shape, bool)
    from_ranks[np.repeat(np.arange(rk.shape[0]), rk.shape[1]), rk.ravel()] = True
    assert np.array_equal(hit, from_ranks)
    # NDCG sums the same non-negative float64 terms in two orders: at most U k roundings of 2^-53 each apart
    for k, x, y in zip(ks, a.NDCG(), t.NDCG()):
        assert abs(x - y) <= hit.shape[0] * k * 2.0 ** -53 * max(x, y)
    X = model_matrix(data)
    ridx, _, rrank = R.uknn_score_topk(X, rec.nbr_idx, rec.nbr_w, data.item_num, targets=targets)
    assert np.array_equal(a._top(), ridx) and np.array_equal(t.ranks(), rrank)
    masked = TargetRankMetric(rec, targets, top=ks, mask_train=True).ranks()
    assert np.array_equal(masked, R.uknn_score_topk(X, rec.nbr_idx, rec.nbr_w, 1, mask_profile=True, targets=targets)[2]) and (masked == -1).any()


def test_neighbour_share_hand_values_on_a_planted_block():
    """Six real users in two groups of three and three fake users that copy group A's items: with 'count' weights every share is a ratio of small
    integers.  Group A = {0, 1, 2} on users a0..a2, group B = {5, 6, 7} on b0..b2 with b2 also holding item 9; the fakes f0..f2 hold {0, 1, 2, 9}."""
    from arlib_amd.util.DataLoader import DataLoader
    rows = {'a0': [0, 1, 2], 'a1': [0, 1, 2], 'a2': [0, 1, 2], 'b0': [5, 6, 7], 'b1': [5, 6, 7], 'b2': [5, 6, 7, 9],
            'f0': [0, 1, 2, 9], 'f1': [0, 1, 2, 9], 'f2': [0, 1, 2, 9]}
    names = list(rows)
    u = np.array([names.index(n) for n in names for _ in rows[n]])
    i = np.array([c for n in names for c in rows[n]])
    data = DataLoader.from_arrays((u, i, np.ones(len(u))), None, (u[:1], i[:1], np.ones(1)), dataName='block', array_native=False)
    from arlib_amd.recommender import UserKNN
    with contextlib.redirect_stdout(io.StringIO()):
        rec = UserKNN(rec_args(knn_k=4, knn_measure='count'), data)
        rec.train()
    assert [data.user[str(r)] for r in range(9)] == list(range(9))                             # internal ids in the order of `names`: ties go by them
    fakes = [str(names.index(n)) for n in ('f0', 'f1', 'f2')]
    share = rec.neighbour_share(fakes)
    assert share.dtype == np.float64 and share.shape == (9,)
    by = {n: share[data.user[str(names.index(n))]] for n in names}
    # a0: the five others with count 3 tie, the four smallest ids are kept: a1, a2, f0, f1 -> fakes hold 6 of 12
    assert by['a0'] == 0.5 and by['a1'] == 0.5 and by['a2'] == 0.5
    # b0, b1: their two group mates only.  b2: b0, b1 with 3 each, f0..f2 with 1 each; k = 4 keeps b0, b1, f0, f1 -> 2 of 8
    assert by['b0'] == 0.0 and by['b1'] == 0.0 and by['b2'] == 0.25
    # f0: f1, f2 with 4, then a0..a2 with 3: keeps f1, f2, a0, a1 -> 8 of 14
    assert by['f0'] == 8 / 14 and by['f1'] == 8 / 14 and by['f2'] == 8 / 14
    assert rec.neighbour_share([]).tolist() == [0.0] * 9 and rec.neighbour_share(['nobody']).tolist() == [0.0] * 9
    assert rec.neighbour_share(list(data.user)).tolist() == [1.0] * 9
    # a user without neighbours: share 0
    rec.nbr_idx = rec.nbr_idx.copy()
    rec.nbr_idx[0] = -1
    assert rec.neighbour_share(fakes)[0] == 0.0


# ------------------------------------------------------------------------------------------------ argument handling
def test_wrapper_raises_value_errors():
    from arlib_amd import userknn
    rp, ci = np.array([0, 2, 3, 3], np.int64), np.array([0, 1, 1], np.int32)
    ni, nw = np.array([[1, -1], [0, 2], [1, -1]], np.int32), np.array([[5, -9], [5, 1], [1, 0]], np.int32)
    ok = dict(rowptr=rp, col=ci, n_users=3, n_items=2, nbr_idx=ni, nbr_w=nw, N=2, route='host')
    idx, score, rank = userknn.uknn_score_topk(**dict(ok, targets=[1, 0]))
    # user 0 lists user 1 = {1} with 5 (the -9 of an unused slot is ignored); user 1 lists user 0 = {0, 1} with 5 and the empty user 2; user 2 lists user 1 with 1
    assert idx.tolist() == [[1, 0], [0, 1], [1, 0]] and score.tolist() == [[5, 0], [5, 5], [1, 0]] and rank.tolist() == [[0, 1], [1, 0], [0, 1]]
    for bad in (dict(N=0), dict(route='fast'), dict(n_users=2), dict(n_users=-1), dict(n_items=1), dict(rowptr=np.array([0, 3, 2, 3])),
                dict(rowptr=np.array([1, 2, 3, 3])), dict(col=np.array([0, -1, 1])), dict(col=np.array([0, 2, 1])), dict(col=np.array([0.0, 1.0, 1.0])),
                dict(rows=[3]), dict(rows=[-1]), dict(rows=[0.5]), dict(rows=np.array([True, False])), dict(tile_items=0),
                dict(tile_items=userknn.UKNN_MAX_TILE_ITEMS + 1), dict(col=np.zeros((3, 1), np.int32)),
                dict(nbr_idx=ni[:2]), dict(nbr_w=nw[:, :1]), dict(nbr_idx=np.array([[1, -1], [0, 3], [1, -1]])), dict(nbr_idx=np.array([[1, -2], [0, 2], [1, -1]])),
                dict(nbr_idx=ni.astype(np.float64)), dict(nbr_idx=np.zeros((3, 0), np.int32), nbr_w=np.zeros((3, 0), np.int32)),
                dict(nbr_w=np.array([[5, 0], [-5, 1], [1, 0]])), dict(nbr_w=np.array([[5, 0], [2 ** 31, 1], [1, 0]], np.int64)),
                dict(targets=[2]), dict(targets=[-1]), dict(targets=[1, 1]), dict(targets=[0.5]), dict(targets=np.zeros((1, 1), np.int64))):
        with pytest.raises(ValueError):
            userknn.uknn_score_topk(**dict(ok, **bad))
    # ids are checked at their own width
    with pytest.raises(ValueError, match='item id'):
        userknn.uknn_score_topk(**dict(ok, col=np.array([0, 2 ** 32 + 1, 1], np.int64)))
    with pytest.raises(ValueError, match='neighbour id'):
        userknn.uknn_score_topk(**dict(ok, nbr_idx=np.array([[1, -1], [0, 2 ** 32 + 1], [1, -1]], np.int64)))
    with pytest.raises(ValueError, match=r'n_users = 3, k'):
        userknn.uknn_score_topk(**dict(ok, nbr_idx=ni[:2], nbr_w=nw[:2]))
    # the kernel's limits: past them 'auto' takes the host route and 'kernel' refuses
    assert userknn.uknn_supported(128, 128, 64) and not userknn.uknn_supported(129, 5) and not userknn.uknn_supported(5, 129) and not userknn.uknn_supported(5, 5, 65)
    assert not userknn.uknn_supported(5, 5, 0, n_queries=2 ** 29) and userknn.uknn_supported(5, 5, 0, n_queries=2 ** 28)
    with pytest.raises(ValueError, match='needs a GPU'):
        userknn.uknn_score_topk(**dict(ok, route='kernel', device='cpu'))
    for bad in (dict(N=0), dict(rows=[3]), dict(targets=[0, 0]), dict(nbr_w=np.array([[5, 0], [-5, 1], [1, 0]])), dict(nbr_idx=ni[:2], nbr_w=nw[:2])):
        with pytest.raises(ValueError):
            userknn.uknn_score_topk_host(**dict(dict(interact=sp.csr_matrix((np.ones(3), ci, rp), shape=(3, 2)), nbr_idx=ni, nbr_w=nw, N=2), **bad))


def test_without_a_gpu_device_auto_takes_the_host_route(planted, monkeypatch):
    """A problem inside the kernel's limits on device='cpu': the C entry must never see host memory."""
    from arlib_amd import _lib, userknn
    X, ni, nw, ref = planted
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was reached'))
    idx, score, rank = userknn.uknn_score_topk(X.indptr, X.indices, 320, 400, ni, nw, 10, targets=TARGETS[5], device='cpu', route='auto')
    col = [TARGETS[64].index(t) for t in TARGETS[5]]
    assert idx.device.type == 'cpu' and np.array_equal(idx.numpy(), ref[False][0][:, :10]) and np.array_equal(rank.numpy(), ref[False][2][:, col])
    # past the limits: N = 200 > 128 goes to the host route whatever the device
    big = userknn.uknn_score_topk(X.indptr, X.indices, 320, 400, ni, nw, 200, device='cpu')
    assert np.array_equal(big[0].numpy()[:, :128], ref[False][0]) and big[0].shape == (320, 200)


def test_c_entry_refuses_each_defect_before_any_launch():
    from arlib_amd import _lib, userknn
    L = _lib.lib()
    assert L.arl_userknn_max_tile_items() == userknn.UKNN_MAX_TILE_ITEMS and L.arl_userknn_default_tile_items() == userknn.UKNN_DEFAULT_TILE_ITEMS
    # the item side's fixed 16 512 bytes and a cursor, an end (64-bit) and a weight (32-bit) for each of 128 slots
    fixed = 16512 + 128 * (8 + 8 + 4)
    assert fixed + 8 * userknn.UKNN_MAX_TILE_ITEMS <= 160 * 1024 < fixed + 8 * (userknn.UKNN_MAX_TILE_ITEMS + 2)
    assert fixed + 8 * userknn.UKNN_DEFAULT_TILE_ITEMS <= 80 * 1024 < fixed + 8 * (userknn.UKNN_DEFAULT_TILE_ITEMS + 2)
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    # 0 rowptr 1 col 2 n_users 3 n_items 4 nbr_idx 5 nbr_w 6 k 7 rows 8 n_queries 9 n 10 mask 11 tgt_id 12 tgt_col 13 n_targets 14 order 15 tile 16 idx 17 score 18 rank 19 stream
    good = [p, p, 4, 4, p, p, 2, None, 4, 3, 0, p, p, 2, None, 0, p, p, p, None]

    def call(**kw):
        a = list(good)
        for pos, v in kw.items():
            a[int(pos[1:])] = v
        return L.arl_userknn_score_topk_i64(*a)
    NULL, RANGE, ARG = -1, -3, -4
    assert call(_0=None) == NULL and call(_4=None) == NULL and call(_5=None) == NULL and call(_16=None) == NULL and call(_17=None) == NULL
    assert call(_11=None) == NULL and call(_12=None) == NULL and call(_18=None) == NULL
    assert call(_2=-1) == ARG and call(_3=-1) == ARG and call(_8=-1) == ARG and call(_6=0) == ARG and call(_9=0) == ARG and call(_13=-1) == ARG and call(_15=-1) == ARG
    assert call(_6=129) == RANGE and call(_9=129) == RANGE and call(_13=65) == RANGE and call(_15=userknn.UKNN_MAX_TILE_ITEMS + 1) == RANGE
    assert call(_2=2 ** 31) == RANGE and call(_3=2 ** 31) == RANGE and call(_8=2 ** 31) == RANGE and call(_8=2 ** 30, _9=2) == RANGE
    assert call(_8=2 ** 30, _9=1, _13=2) == RANGE
    assert call(_8=0, _0=None, _16=None, _17=None, _18=None) == 0                                # no queries: nothing to do


def test_abi_version_and_the_new_exports():
    from arlib_amd import _lib
    assert _lib.ABI_VERSION == 34 and _lib.lib().arl_abi_version() == 34
    for name in ('arl_userknn_score_topk_i64', 'arl_userknn_max_tile_items', 'arl_userknn_default_tile_items'):
        assert name in _lib.EXPORTS and hasattr(_lib.lib(), name)
    assert _lib._SIGS['arl_userknn_score_topk_i64'] == _lib._SIGS['arl_itemknn_score_topk_i64']          # the same argument list

"""arl_itemknn_score_topk_i64 through arlib_amd.itemknn.knn_score_topk on the GPU, against the pure-Python restatement
(tests/itemknn_restatement.py) and, past the sizes that one reaches, against the host route.  Every comparison is array_equal: the scores are
exact int64 sums and the order is decided in integers, so there is no tolerance anywhere."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import itemknn_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TILES = (None, 64, 100)                                     # the default (one tile here) / 400 items in 6 whole tiles and a ragged one of 16 / 4 whole tiles
TARGETS = [390, 391, 392] + [i for i in range(0, 400, 6) if i not in (390, 391, 392)][:61]      # 64 ids, not in ascending order


def run(X, ni, nw, N, rows=None, mask=False, targets=None, tile_items=None):
    from arlib_amd import itemknn
    X = sp.csr_matrix(X)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    idx, score, rank = itemknn.knn_score_topk(t(X.indptr, np.int64), t(X.indices, np.int32), X.shape[0], X.shape[1], t(ni, np.int32), t(nw, np.int32), N,
                                              rows=rows, mask_profile=mask, targets=targets, tile_items=tile_items, route='kernel')
    assert idx.is_cuda and idx.dtype == torch.int32 and score.dtype == torch.int64 and idx.shape == score.shape
    assert (rank is None) == (targets is None) and (rank is None or rank.dtype == torch.int32)
    return idx.cpu().numpy(), score.cpu().numpy(), None if rank is None else rank.cpu().numpy()


def same(got, ref, N=None, cols=None):
    return (np.array_equal(got[0], ref[0] if N is None else ref[0][:, :N]) and np.array_equal(got[1], ref[1] if N is None else ref[1][:, :N])
            and (got[2] is None or np.array_equal(got[2], ref[2] if cols is None else ref[2][:, cols])))


@pytest.fixture(scope='module')
def planted():
    """The planted 320 x 400 input, its restated lists at k = 1, 7, 128 and the restated results at N = 128 with the 64 targets."""
    X, _ = R.planted()
    lists = {k: R.lists_of(X, k, 'cosine') for k in (1, 7, 128)}
    ref = {(k, m): R.knn_score_topk(X, lists[k][0], lists[k][1], 128, mask_profile=m, targets=TARGETS) for k in (1, 7, 128) for m in (False, True)}
    return X, lists, ref


@pytest.mark.parametrize('tile_items', TILES)
@pytest.mark.parametrize('k', [1, 7, 128])
def test_planted_input_equals_the_restatement(planted, k, tile_items):
    X, lists, ref = planted
    assert X.shape == (320, 400)
    ni, nw = lists[k]
    if k == 128:
        assert (ni == -1).any()                             # unused slots
    for mask in (False, True):
        for N in (1, 10, 128):
            assert same(run(X, ni, nw, N, mask=mask, targets=TARGETS, tile_items=tile_items), ref[(k, mask)], N), (mask, N)
    got = run(X, ni, nw, 10, mask=True, tile_items=tile_items)          # no targets: no rank
    assert got[2] is None and same(got, ref[(k, True)], 10)
    for T in (1, 5):
        assert same(run(X, ni, nw, 10, mask=True, targets=TARGETS[:T], tile_items=tile_items), ref[(k, True)], 10, list(range(T)))
    masked = run(X, ni, nw, 1, mask=True, targets=TARGETS[:3], tile_items=tile_items)[2]
    assert (masked[300:] == -1).all() and (masked[:300] >= -1).all()    # the fake rows hold 390..392


def test_rows_subset_repeats_and_no_queries(planted):
    X, lists, ref = planted
    ni, nw = lists[7]
    rows = np.random.RandomState(5).permutation(320)[:77]
    rows[40] = rows[3]
    rows[9] = 311
    for tile_items in TILES:
        got = run(X, ni, nw, 9, rows=torch.from_numpy(rows), mask=True, targets=TARGETS, tile_items=tile_items)
        r = ref[(7, True)]
        assert np.array_equal(got[0], r[0][rows, :9]) and np.array_equal(got[1], r[1][rows, :9]) and np.array_equal(got[2], r[2][rows])
    none = run(X, ni, nw, 9, rows=np.zeros(0, np.int64), targets=TARGETS[:2])
    assert none[0].shape == (0, 9) and none[1].shape == (0, 9) and none[2].shape == (0, 2)


def test_carry_past_32_bits():
    """9 profile items each list item 20 with weight 2^30: 9 * 2^30; item 21 receives 2^31 - 1 from each of 3 lists."""
    I = 30
    ni, nw = np.full((I, 2), -1, np.int32), np.zeros((I, 2), np.int32)
    ni[:9, 0], nw[:9, 0] = 20, 2 ** 30
    ni[:3, 1], nw[:3, 1] = 21, 2 ** 31 - 1
    X = sp.csr_matrix((np.ones(9 + 2, np.int64), (np.r_[np.zeros(9, np.int64), 1, 1], np.r_[np.arange(9), 0, 1])), shape=(2, I))
    for tile_items in (None, 7):
        idx, score, rank = run(X, ni, nw, 3, targets=[21, 20, 5], tile_items=tile_items)
        assert idx[0].tolist() == [20, 21, 0] and score[0].tolist() == [9 * 2 ** 30, 3 * (2 ** 31 - 1), 0] and rank[0].tolist() == [1, 0, 7]
        assert idx[1].tolist() == [21, 20, 0] and score[1].tolist() == [2 * (2 ** 31 - 1), 2 * 2 ** 30, 0] and rank[1].tolist() == [0, 1, 7]
        assert same((idx, score, rank), R.knn_score_topk(X, ni, nw, 3, targets=[21, 20, 5]))


@pytest.mark.parametrize('tile_items', (None, 16))
def test_tie_rule_on_identical_rows(tile_items):
    """All weights equal on identical_rows(): every listed item ties, so the lists are the smallest unmasked ids in order."""
    X = R.identical_rows()
    held = [1, 5, 8, 13, 21, 34]
    ni = np.tile(np.array([i for i in range(40) if i not in (3, 17)], np.int32), (40, 1))          # every item lists the same 38 items
    nw = np.full(ni.shape, 5, np.int32)
    idx, score, rank = run(X, ni, nw, 12, targets=[3, 0, 39], tile_items=tile_items)
    best = [i for i in range(40) if i not in (3, 17)]
    assert (idx == np.array(best[:12])).all() and (score == 30).all()
    assert (rank == np.array([38, 0, 37])).all()            # 3 scores 0: behind the 38 listed items; 39 is the last of those
    idx, score, rank = run(X, ni, nw, 12, mask=True, targets=[3, 0, 5], tile_items=tile_items)
    assert (idx == np.array([i for i in best if i not in held][:12])).all() and (rank == np.array([32, 0, -1])).all()
    assert same((idx, score, rank), R.knn_score_topk(X, ni, nw, 12, mask_profile=True, targets=[3, 0, 5]))


def test_degenerate_profiles_and_a_small_catalogue():
    """An empty profile (all scores 0, the list is ids 0..N-1), a user holding every item with masking (all -1, every rank -1), and a catalogue
    of 40 items with N = 128 (the padding is written)."""
    rng = np.random.RandomState(3)
    I = 40
    D = (rng.random_sample((6, I)) < 0.2).astype(np.int64)
    D[2] = 0
    D[4] = 1
    X = sp.csr_matrix(D)
    ni = rng.randint(-1, I, (I, 5)).astype(np.int32)
    nw = rng.randint(0, 2 ** 31 - 1, (I, 5)).astype(np.int32)
    tg = [7, 0, 39, 22]
    for tile_items in (None, 16, 13):
        for mask in (False, True):
            got = run(X, ni, nw, 128, mask=mask, targets=tg, tile_items=tile_items)
            assert same(got, R.knn_score_topk(X, ni, nw, 128, mask_profile=mask, targets=tg))
            assert (got[0][:, I:] == -1).all() and (got[1][:, I:] == 0).all()
            assert got[0][2, :I].tolist() == list(range(I)) and (got[1][2] == 0).all() and got[2][2].tolist() == [7, 0, 39, 22]
        assert (got[0][4] == -1).all() and (got[1][4] == 0).all() and (got[2][4] == -1).all()
    got = run(X, ni, nw, 5, rows=[2, 2], tile_items=16)
    assert got[0].tolist() == [[0, 1, 2, 3, 4]] * 2


def test_long_profile_over_several_tiles_and_targets_past_the_first_tile():
    """A profile of 600 items over several tiles; every target lies in a tile other than the first."""
    from arlib_amd import itemknn
    rng = np.random.RandomState(12)
    I = 900
    D = (rng.random_sample((12, I)) < 0.03).astype(np.int64)
    D[5, :] = 0
    D[5, rng.permutation(I)[:600]] = 1
    X = sp.csr_matrix(D)
    ni = rng.randint(-1, I, (I, 9)).astype(np.int32)
    ni[:, 3] = ni[:, 2]                                     # a neighbour named twice in one list: both weights count
    nw = rng.randint(0, 2 ** 31 - 1, (I, 9)).astype(np.int32)
    tg = [899, 300, 512, 256, 640]
    ref = {m: R.knn_score_topk(X, ni, nw, 128, mask_profile=m, targets=tg) for m in (False, True)}
    for mask in (False, True):
        host = itemknn.knn_score_topk_host(X, ni, nw, 128, mask_profile=mask, targets=tg)
        assert same(host, ref[mask])
        for tile_items in (None, 256, 100):
            assert same(run(X, ni, nw, 128, mask=mask, targets=tg, tile_items=tile_items), ref[mask]), (mask, tile_items)


def test_default_tile_seam_against_the_host_route():
    from arlib_amd import itemknn
    I = itemknn.KNN_DEFAULT_TILE_ITEMS + 37
    rng = np.random.RandomState(3)
    U = 24
    r, c = np.repeat(np.arange(U), 30), rng.randint(0, I, 30 * U)
    X = sp.csr_matrix((np.ones(30 * U, np.int64), (r, c)), shape=(U, I))
    X.sum_duplicates()
    ni = rng.randint(0, I, (I, 6)).astype(np.int32)
    ni[:, 5] = np.where(rng.random_sample(I) < 0.5, I - 1 - rng.randint(0, 40, I), ni[:, 5])       # entries past the seam
    nw = rng.randint(0, 2 ** 30, (I, 6)).astype(np.int32)
    tg = [I - 1, itemknn.KNN_DEFAULT_TILE_ITEMS, itemknn.KNN_DEFAULT_TILE_ITEMS - 1, 5]
    for mask in (False, True):
        assert same(run(X, ni, nw, 50, mask=mask, targets=tg), itemknn.knn_score_topk_host(X, ni, nw, 50, mask_profile=mask, targets=tg))


def test_two_runs_give_the_same_bits(planted):
    X, lists, _ = planted
    ni, nw = lists[7]
    a, b = run(X, ni, nw, 32, mask=True, targets=TARGETS, tile_items=64), run(X, ni, nw, 32, mask=True, targets=TARGETS, tile_items=64)
    assert same(a, b)


def test_the_kernel_route_refuses_what_is_past_its_limits(planted):
    from arlib_amd import itemknn
    X, lists, ref = planted
    ni, nw = lists[7]
    with pytest.raises(ValueError, match='knn_score_topk_host'):
        run(X, ni, nw, 129)
    with pytest.raises(ValueError, match='knn_score_topk_host'):
        run(X, ni, nw, 5, targets=list(range(65)))
    idx, _, _ = itemknn.knn_score_topk(X.indptr, X.indices, 320, 400, ni, nw, 200, device=DEV, route='auto')       # 'auto': the host route
    assert idx.shape == (320, 200) and np.array_equal(idx.numpy()[:, :128], ref[(7, False)][0])


def test_itemknn_model_on_the_gpu_equals_the_host_route():
    from test_itemknn_cpu import synthetic_data, rec_args
    from arlib_amd.recommender import ItemKNN
    from arlib_amd.util.metrics import AttackMetric, TargetRankMetric
    data = synthetic_data()
    out = {}
    for route in ('kernel', 'host'):
        with contextlib.redirect_stdout(io.StringIO()):
            rec = ItemKNN(rec_args(knn_route=route), data)
            rec.train()
            rec_list, measure = rec.test()
        tg = [3, 40, 17]
        out[route] = (rec.nbr_idx, rec.nbr_w, rec_list, measure, rec.bestPerformance, AttackMetric(rec, tg, top=[5, 20])._top(),
                      TargetRankMetric(rec, tg, mask_train=True).ranks())
    k, h = out['kernel'], out['host']
    assert np.array_equal(k[0], h[0]) and np.array_equal(k[1], h[1])
    assert k[2] == h[2] and k[3] == h[3] and k[4] == h[4]   # the lists, float scores included, the measure strings, bestPerformance: bit for bit
    assert np.array_equal(k[5], h[5]) and np.array_equal(k[6], h[6])

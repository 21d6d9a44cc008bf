"""arl_userknn_score_topk_i64 through arlib_amd.userknn.uknn_score_topk on the GPU, against the pure-Python restatement
(tests/userknn_restatement.py) on its planted 60 x 150 input and, past the sizes that one reaches, against the host route.  Every comparison is
array_equal: the scores are exact int64 sums and the order is decided in integers, so there is no tolerance anywhere."""
import contextlib
import io

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import userknn_restatement as R

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TILES = (None, 16, 64)                                      # the default (one tile here) / 9 whole tiles and a ragged one of 6 / 2 whole tiles and one of 22
# 64 ids, not in ascending order: the fake rows' targets (masked there, in the last tile at both tile sizes), then every other even id
TARGETS = [140, 141, 149] + [i for i in range(0, 150, 2) if i not in (140,)][:61]


def run(X, ni, nw, N, rows=None, mask=False, targets=None, tile_items=None):
    from arlib_amd import userknn
    X = sp.csr_matrix(X)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(DEV)
    idx, score, rank = userknn.uknn_score_topk(t(X.indptr, np.int64), t(X.indices, np.int32), X.shape[0], X.shape[1], t(ni, np.int32), t(nw, np.int32), N,
                                               rows=rows, mask_profile=mask, targets=targets, tile_items=tile_items, route='kernel')
    assert idx.is_cuda and idx.dtype == torch.int32 and score.dtype == torch.int64 and idx.shape == score.shape
    assert (rank is None) == (targets is None) and (rank is None or rank.dtype == torch.int32)
    return idx.cpu().numpy(), score.cpu().numpy(), None if rank is None else rank.cpu().numpy()


def same(got, ref, N=None, cols=None):
    return (np.array_equal(got[0], ref[0] if N is None else ref[0][:, :N]) and np.array_equal(got[1], ref[1] if N is None else ref[1][:, :N])
            and (got[2] is None or np.array_equal(got[2], ref[2] if cols is None else ref[2][:, cols])))


@pytest.fixture(scope='module')
def planted():
    """The planted 60 x 150 input, its restated lists at k = 1, 7, 128 and the restated results at N = 128 with the 64 targets."""
    X = R.small()
    lists = {k: R.lists_of(X, k, 'cosine') for k in (1, 7, 128)}
    ref = {(k, m): R.uknn_score_topk(X, lists[k][0], lists[k][1], 128, mask_profile=m, targets=TARGETS) for k in (1, 7, 128) for m in (False, True)}
    return X, lists, ref


@pytest.mark.parametrize('tile_items', TILES)
@pytest.mark.parametrize('k', [1, 7, 128])
def test_planted_input_equals_the_restatement(planted, k, tile_items):
    X, lists, ref = planted
    assert X.shape == (60, 150) and len(set(TARGETS)) == 64
    ni, nw = lists[k]
    if k == 128:
        assert (ni == -1).any() and (ni[:, 40] >= 0).any()  # more slots than users: unused slots behind long lists
    if k == 1:
        assert (ref[(1, False)][1][:, 40] == 0).sum() > 30  # one neighbour: for most users most of the catalogue, targets included, is held by no neighbour
    for mask in (False, True):
        for N in (1, 10, 128):
            assert same(run(X, ni, nw, N, mask=mask, targets=TARGETS, tile_items=tile_items), ref[(k, mask)], N), (mask, N)
    got = run(X, ni, nw, 10, mask=True, tile_items=tile_items)          # no targets: no rank
    assert got[2] is None and same(got, ref[(k, True)], 10)
    for T in (1, 5):
        assert same(run(X, ni, nw, 10, mask=True, targets=TARGETS[:T], tile_items=tile_items), ref[(k, True)], 10, list(range(T)))
    masked = run(X, ni, nw, 1, mask=True, targets=TARGETS[:3], tile_items=tile_items)[2]
    assert (masked[52:] == -1).all() and (masked[41] == -1).all() and (masked[:40] >= -1).all()      # the fake rows and the full row hold 140, 141, 149
    # the empty profile is a query like any other (nothing is masked); the profile holding the whole catalogue has no candidate
    full = run(X, ni, nw, 5, rows=[41, 40], mask=True, targets=TARGETS[:3], tile_items=tile_items)
    assert (full[0][0] == -1).all() and (full[1][0] == 0).all() and (full[2][0] == -1).all()
    assert (full[0][1] >= 0).all() and (full[2][1] >= 0).all()


@pytest.mark.parametrize('tile_items', TILES)
def test_cursor_and_chunk_seams(tile_items):
    """Every user lists the seam rows of R.small(): the empty row 40, the full row 41 (150 entries: chunks of 64, 64 and 22), row 42 with entries
    at 15 and 16 (t1 - 1 and t1 of the first tile of 16), row 43 ending exactly at item 15, row 44 with no entry between 3 and 100, and rows
    45..48 of 63, 64, 65 and 128 consecutive entries from item 7 (a chunk that ends one short of, exactly at and one past the 64 lanes, and two
    whole chunks; at tile 64 row 45 ends at item 69 and row 48 crosses two seams).  Each slot has its own weight, so a wrong cursor shows."""
    X = R.small()
    ni = np.tile(np.arange(40, 49, dtype=np.int32), (60, 1))
    nw = (np.arange(60)[:, None] * 131 + 2 ** np.arange(9)[None, :] * 1009).astype(np.int32)
    for mask in (False, True):
        ref = R.uknn_score_topk(X, ni, nw, 128, mask_profile=mask, targets=TARGETS)
        assert same(run(X, ni, nw, 128, mask=mask, targets=TARGETS, tile_items=tile_items), ref), mask
    # the lists in another slot order, with unused slots between them, a slot naming the query itself and a neighbour in two slots
    rng = np.random.RandomState(2)
    ni2 = np.full((60, 14), -1, np.int32)
    for u in range(60):
        ni2[u, rng.permutation(14)[:9]] = rng.permutation(np.arange(40, 49))
        ni2[u, np.flatnonzero(ni2[u] < 0)[:2]] = (u, 45)
    nw2 = rng.randint(0, 2 ** 31 - 1, ni2.shape).astype(np.int32)
    assert (ni2 == -1).any() and all(u in ni2[u] for u in range(60))
    ref = R.uknn_score_topk(X, ni2, nw2, 20, mask_profile=True, targets=TARGETS[:7])
    assert same(run(X, ni2, nw2, 20, mask=True, targets=TARGETS[:7], tile_items=tile_items), ref)


def test_rows_subset_repeats_and_no_queries(planted):
    X, lists, ref = planted
    ni, nw = lists[7]
    rows = np.random.RandomState(5).permutation(60)[:33]
    rows[20] = rows[3]
    rows[9] = 55
    for tile_items in TILES:
        got = run(X, ni, nw, 9, rows=torch.from_numpy(rows), mask=True, targets=TARGETS, tile_items=tile_items)
        r = ref[(7, True)]
        assert np.array_equal(got[0], r[0][rows, :9]) and np.array_equal(got[1], r[1][rows, :9]) and np.array_equal(got[2], r[2][rows])
    none = run(X, ni, nw, 9, rows=np.zeros(0, np.int64), targets=TARGETS[:2])
    assert none[0].shape == (0, 9) and none[1].shape == (0, 9) and none[2].shape == (0, 2)


def test_carry_past_32_bits():
    """128 slots of weight 2^31 - 1, all naming row 43 = {0..15}: 128 (2^31 - 1) on each of its items; 3 of the slots of user 1 name row 42 = {15, 16}."""
    X = R.small()
    ni, nw = np.full((60, 128), 43, np.int32), np.full((60, 128), 2 ** 31 - 1, np.int32)
    ni[1, 5:8] = 42
    big = 2 ** 31 - 1
    for tile_items in (None, 16):
        idx, score, rank = run(X, ni, nw, 18, rows=[0, 1], targets=[16, 15, 17], tile_items=tile_items)
        assert idx[0].tolist() == list(range(18)) and score[0].tolist() == [128 * big] * 16 + [0, 0] and rank[0].tolist() == [16, 15, 17]
        assert idx[1].tolist() == [15] + list(range(15)) + [16, 17] and score[1].tolist() == [128 * big] + [125 * big] * 15 + [3 * big, 0]
        assert rank[1].tolist() == [16, 0, 17]
        assert same((idx, score, rank), R.uknn_score_topk(X, ni, nw, 18, rows=[0, 1], targets=[16, 15, 17]))


@pytest.mark.parametrize('tile_items', (None, 16))
def test_tie_rule_on_identical_rows_and_a_small_catalogue(tile_items):
    """Identical rows: every neighbour brings the same six items with the same weight, so the held items tie and the rest ties at 0; the lists
    are decided by the id alone.  40 items with N = 128: the padding is written."""
    X = R.identical_rows(60, 40)
    held = [1, 5, 8, 13, 21, 34]
    ni, nw = R.lists_of(X, 5, 'count')
    assert (nw == 6).all() and ni[0].tolist() == [1, 2, 3, 4, 5]
    rest = [i for i in range(40) if i not in held]
    idx, score, rank = run(X, ni, nw, 128, targets=[3, 0, 34, 39], tile_items=tile_items)
    assert (idx[:, :40] == np.array(held + rest)).all() and (score[:, :6] == 30).all() and (score[:, 6:] == 0).all() and (idx[:, 40:] == -1).all()
    assert (rank == np.array([8, 6, 5, 39])).all()
    idx, score, rank = run(X, ni, nw, 128, mask=True, targets=[3, 0, 34, 39], tile_items=tile_items)
    assert (idx[:, :34] == np.array(rest)).all() and (idx[:, 34:] == -1).all() and (score == 0).all() and (rank == np.array([2, 0, -1, 33])).all()
    assert same((idx, score, rank), R.uknn_score_topk(X, ni, nw, 128, mask_profile=True, targets=[3, 0, 34, 39]))


@pytest.mark.parametrize('shape', ['below', 'above', 'two_and_ragged'])
def test_default_tile_seam_against_the_host_route(shape):
    from arlib_amd import userknn
    D = userknn.UKNN_DEFAULT_TILE_ITEMS
    I = {'below': D - 1, 'above': D + 1, 'two_and_ragged': 2 * D + 37}[shape]
    rng = np.random.RandomState(3)
    U = 40
    seam = np.r_[np.arange(D - 3, min(D + 3, I)), np.arange(max(I - 3, 0), I)]        # entries on both sides of the seam and at the catalogue's end
    r = np.r_[np.repeat(np.arange(U), 30), np.repeat(np.arange(0, U, 2), len(seam))]
    c = np.r_[rng.randint(0, I, 30 * U), np.tile(seam, U // 2)]
    X = sp.csr_matrix((np.ones(len(r), np.int64), (r, c)), shape=(U, I))
    X.sum_duplicates()
    ni = rng.randint(-1, U, (U, 6)).astype(np.int32)
    nw = rng.randint(0, 2 ** 30, (U, 6)).astype(np.int32)
    tg = list(dict.fromkeys([I - 1, min(D, I - 2), D - 2, D - 3, 5]))                 # on both sides of the seam where the catalogue has both
    for mask in (False, True):
        assert same(run(X, ni, nw, 50, mask=mask, targets=tg), userknn.uknn_score_topk_host(X, ni, nw, 50, mask_profile=mask, targets=tg)), mask


def test_two_runs_give_the_same_bits(planted):
    X, lists, _ = planted
    ni, nw = lists[7]
    a, b = run(X, ni, nw, 32, mask=True, targets=TARGETS, tile_items=16), run(X, ni, nw, 32, mask=True, targets=TARGETS, tile_items=16)
    assert same(a, b)


def test_the_kernel_route_refuses_what_is_past_its_limits(planted):
    from arlib_amd import userknn
    X, lists, ref = planted
    ni, nw = lists[7]
    with pytest.raises(ValueError, match='uknn_score_topk_host'):
        run(X, ni, nw, 129)
    with pytest.raises(ValueError, match='uknn_score_topk_host'):
        run(X, ni, nw, 5, targets=list(range(65)))
    with pytest.raises(ValueError, match='uknn_score_topk_host'):
        run(X, np.tile(ni[:, :1], (1, 129)), np.tile(nw[:, :1], (1, 129)), 5)
    with pytest.raises(ValueError, match='tile_items'):
        run(X, ni, nw, 5, tile_items=userknn.UKNN_MAX_TILE_ITEMS + 1)
    idx, _, _ = userknn.uknn_score_topk(X.indptr, X.indices, 60, 150, ni, nw, 140, device=DEV, route='auto')        # 'auto': the host route
    assert idx.shape == (60, 140) and np.array_equal(idx.numpy()[:, :128], ref[(7, False)][0])


def test_userknn_model_on_the_gpu_equals_the_host_route():
    from test_userknn_cpu import synthetic_data, rec_args
    from arlib_amd.recommender import UserKNN
    from arlib_amd.util.metrics import AttackMetric, TargetRankMetric
    data = synthetic_data()
    out = {}
    for route in ('kernel', 'host'):
        with contextlib.redirect_stdout(io.StringIO()):
            rec = UserKNN(rec_args(knn_route=route), data)
            rec.train()
            rec_list, measure = rec.test()
        tg = [3, 40, 17]
        fakes = list(data.user)[-5:]
        out[route] = (rec.nbr_idx, rec.nbr_w, rec_list, measure, rec.bestPerformance, AttackMetric(rec, tg, top=[5, 20])._top(),
                      TargetRankMetric(rec, tg, mask_train=True).ranks(), rec.neighbour_share(fakes))
    k, h = out['kernel'], out['host']
    assert np.array_equal(k[0], h[0]) and np.array_equal(k[1], h[1])
    assert k[2] == h[2] and k[3] == h[3] and k[4] == h[4]   # the lists, float scores included, the measure strings, bestPerformance: bit for bit
    assert np.array_equal(k[5], h[5]) and np.array_equal(k[6], h[6]) and np.array_equal(k[7], h[7])

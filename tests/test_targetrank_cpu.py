"""The target-rank op without a GPU: the float64 restatement (tests/rank_restatement.py) against a plain argsort, the tightness of its bracket on the
fixed cases, target_rank_composed on CPU tensors, util.metrics.TargetRankMetric on a stub model, and the argument handling of every layer."""
import os
import re

import numpy as np
import pytest
import torch
import rank_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 10, 50, 500)
_CACHE = {}


def case(k, masked, integer=False):
    """(Pu, Pi, targets, mask | None, restatement) of fixed case k, computed once and shared (never modified)."""
    key = (k, masked, integer)
    if key not in _CACHE:
        U, I, T, d, seed = R.CASES[k]
        Pu, Pi, targets = R.draw_case(U, I, T, d, seed, integer)
        mask = R.draw_mask(U, I, targets, seed) if masked else None
        _CACHE[key] = (Pu, Pi, targets, mask, R.restate(Pu, Pi, targets, mask))
    return _CACHE[key]


def tens(a, dev='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def composed(k, masked, integer=False):
    from arlib_amd import targetrank
    Pu, Pi, targets, mask, ref = case(k, masked, integer)
    rank, ts = targetrank.target_rank_composed(tens(Pu), tens(Pi), tens(targets), (tens(mask[0]), tens(mask[1])) if masked else None)
    assert rank.dtype == torch.int32 and ts.dtype == torch.float32 and rank.shape == ts.shape == (Pu.shape[0], len(targets))
    return rank.numpy(), ts.numpy(), ref


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize('integer', [False, True])
def test_restated_rank_is_the_position_in_a_stable_descending_sort(integer):
    for k in (0, 1, 5):
        Pu, Pi, targets, mask, ref = case(k, True, integer)
        S = Pu.astype(np.float64) @ Pi.astype(np.float64).T
        M = R.dense_mask(mask[0], mask[1], *S.shape)
        for u in range(S.shape[0]):
            keep = np.flatnonzero(~M[u])
            order = keep[np.argsort(-S[u, keep], kind='stable')]            # ties keep ascending item id
            pos = {int(j): r for r, j in enumerate(order)}
            for t, tg in enumerate(targets.tolist()):
                assert ref['rank0'][u, t] == pos.get(tg, -1)
        assert (ref['lo'] <= ref['hi']).all()
        v = ~ref['listed']
        assert ((ref['lo'] <= ref['rank0']) & (ref['rank0'] <= ref['hi']))[v].all()


def test_mask_cases_list_targets_all_targets_and_nothing():
    for k in range(1, len(R.CASES)):
        U, I, T, d, seed = R.CASES[k]
        _, _, targets, (rowptr, col), ref = case(k, True)
        assert ref['listed'][0].all() and rowptr[2] == rowptr[1]                 # user 0 lists every target, user 1 nothing
        assert 0 < ref['listed'][2:].sum() < ref['listed'][2:].size
        assert np.diff(rowptr).max() <= 40 + T
        for u in range(U):
            assert (np.diff(col[rowptr[u]:rowptr[u + 1]]) > 0).all()


def test_the_cases_are_tight():
    """The bracket must not be able to hide a wrong count: over all pairs of every random case hi - lo is at most 2 and 0.1 on average."""
    worst, total, n = 0, 0, 0
    for k in range(len(R.CASES)):
        for masked in (False, True):
            ref = case(k, masked)[4]
            gap = (ref['hi'] - ref['lo'])[~ref['listed']]
            if gap.size:
                worst, total, n = max(worst, int(gap.max())), total + int(gap.sum()), n + gap.size
                print('%s masked %d: max gap %d, mean %.4f' % (R.IDS[k], masked, gap.max(), gap.mean()))
                assert gap.mean() <= 0.1
    print('all: max %d, mean %.4f' % (worst, total / n))
    assert worst <= 2 and total / n <= 0.1


# ------------------------------------------------------------------------------------------------ the composed route on CPU tensors
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', range(len(R.CASES)), ids=R.IDS)
def test_composed_on_cpu_lies_in_the_bracket(k, masked):
    rank, ts, ref = composed(k, masked)
    assert R.check_bracket(rank, ref) == []
    assert (np.abs(ts.astype(np.float64) - ref['tscore']) <= ref['tbound']).all()


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', range(len(R.CASES)), ids=R.IDS)
def test_composed_on_cpu_is_exact_on_integer_tables(k, masked):
    rank, ts, ref = composed(k, masked, integer=True)
    assert np.array_equal(rank, ref['rank0'])
    assert np.array_equal(ts.astype(np.float64), ref['tscore'])
    assert np.array_equal(rank == -1, ref['listed'])


# ------------------------------------------------------------------------------------------------ the metric
class _StubData(object):
    def __init__(self, U, I, mask):
        import scipy.sparse as sp
        self.user = {'u%d' % u: u for u in range(U)}
        self.item = {'i%d' % i: i for i in range(I)}
        rowptr, col = mask
        self._m = sp.csr_matrix((np.ones(len(col), np.float32), col, rowptr), shape=(U, I))

    def matrix(self):
        return self._m


class StubModel(object):
    def __init__(self, Pu, Pi, mask, dev='cpu'):
        self.data = _StubData(Pu.shape[0], Pi.shape[0], mask)
        self.user_emb, self.item_emb = tens(Pu, dev), tens(Pi, dev)


def hold_metric(metric, ref, ks, exact):
    """Each number between the float64 formula at hi and at lo (all four reference metrics, exposure and MRR do not increase with a rank; the mean
    rank does not decrease); on an integer case equal to the formula at the exact ranks."""
    got = {'hitRate': metric.hitRate(), 'precision': metric.precision(), 'recall': metric.recall(), 'NDCG': metric.NDCG(), 'exposure': metric.exposure(),
           'meanRank': metric.meanRank(), 'MRR': metric.MRR()}
    v = ~ref['listed']
    assert np.array_equal(metric.ranks() == -1, ref['listed']) and metric.ranks().dtype == np.int32
    at_lo, at_hi, at_0 = (R.metrics_from_ranks(ref[name], ks, v) for name in ('lo', 'hi', 'rank0'))

    def between(x, a, b):
        if np.isnan(a) or np.isnan(b):
            return np.isnan(x)
        return min(a, b) - 1e-12 <= x <= max(a, b) + 1e-12
    for name, val in got.items():
        if isinstance(val, list):
            assert len(val) == len(ks)
            for q in range(len(ks)):
                assert between(val[q], at_hi[name][q], at_lo[name][q]), (name, ks[q], val[q], at_hi[name][q], at_lo[name][q])
                if exact:
                    assert between(val[q], at_0[name][q], at_0[name][q]), (name, ks[q], val[q], at_0[name][q])
        else:
            assert between(val, at_hi[name], at_lo[name]), (name, val, at_hi[name], at_lo[name])
            if exact:
                assert between(val, at_0[name], at_0[name]), (name, val, at_0[name])


@pytest.mark.parametrize('integer', [False, True], ids=['normal', 'integer'])
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', [1, 5], ids=[R.IDS[1], R.IDS[5]])
def test_metric_on_a_stub_model_lies_in_the_float64_intervals(k, masked, integer):
    from arlib_amd.util.metrics import TargetRankMetric
    Pu, Pi, targets, _, ref = case(k, masked, integer)
    mask = R.draw_mask(Pu.shape[0], Pi.shape[0], targets, R.CASES[k][4])
    ks = [q for q in KS if q <= Pi.shape[0]] + [Pi.shape[0]]
    metric = TargetRankMetric(StubModel(Pu, Pi, mask), targets.tolist(), top=ks, mask_train=masked)
    hold_metric(metric, ref, ks, integer)
    per_target = metric.exposure(per_target=True)
    assert len(per_target) == len(ks) and per_target[0].shape == (len(targets),)


def test_metric_at_k_equal_to_the_catalogue_counts_every_valid_pair():
    from arlib_amd.util.metrics import TargetRankMetric
    Pu, Pi, targets, mask, ref = case(1, True)
    U, I, T = Pu.shape[0], Pi.shape[0], len(targets)
    m = TargetRankMetric(StubModel(Pu, Pi, mask), targets.tolist(), top=[I], mask_train=True)
    n_valid = int((~ref['listed']).sum())
    assert m.recall() == [n_valid / (U * T)] and m.precision() == [n_valid / (U * I)] and m.exposure() == [1.0]


# ------------------------------------------------------------------------------------------------ arguments
def test_argument_handling():
    from arlib_amd import targetrank as tr
    Pu, Pi = torch.randn(6, 16), torch.randn(9, 16)
    ok = torch.tensor([1, 4], dtype=torch.int32)
    rank, _ = tr.target_rank_composed(Pu, Pi, ok)
    assert rank.shape == (6, 2)
    assert tr.target_rank_composed(Pu, Pi, [1, 4])[0].equal(rank)                   # a plain list of ids is taken too
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, torch.tensor([1, 1], dtype=torch.int32))    # duplicate targets
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, torch.tensor([1, 9], dtype=torch.int32))    # a target >= I
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, torch.tensor([-1], dtype=torch.int32))
    with pytest.raises(ValueError):
        tr.target_rank_composed(Pu, Pi, torch.zeros(0, dtype=torch.int32))          # T = 0
    with pytest.raises(TypeError):
        tr.target_rank_composed(Pu, Pi, torch.tensor([1, 4]))                       # int64 ids
    rowptr = torch.tensor([0, 2, 1, 3, 3, 3, 3], dtype=torch.int32)
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, ok, (rowptr, torch.tensor([0, 1, 2], dtype=torch.int32)))      # a rowptr that decreases
    rowptr = torch.tensor([0, 2, 3, 3, 3, 3, 3], dtype=torch.int32)
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, ok, (rowptr, torch.tensor([3, 3, 2], dtype=torch.int32)))      # a row that repeats an item
    with pytest.raises(IndexError):
        tr.target_rank_composed(Pu, Pi, ok, (rowptr, torch.tensor([3, 9, 2], dtype=torch.int32)))      # a column >= I
    with pytest.raises(ValueError):
        tr.target_rank_composed(Pu, Pi, ok, (rowptr, None))                         # a missing mask half
    with pytest.raises(ValueError):
        tr.target_rank_composed(Pu, torch.randn(9, 32), ok)
    # the kernel entry: tables that are not on the GPU are refused before anything else, as by the other ops
    from arlib_amd._lib import ArlError
    with pytest.raises(ArlError):
        tr.target_rank_kernel(Pu, Pi, ok)
    # limits, host only
    assert tr.TARGETRANK_WIDTHS == (16, 32, 64, 128) and tr.TARGETRANK_MAX_TARGETS == 64 and tr.TARGETRANK_MAX_ROWS == (2 ** 31 - 1) // 128
    assert tr.target_rank_supported(1_000_000, 100_000, 64, 5, 32_000_000) and tr.target_rank_supported(1, 1, 16, 1) and tr.target_rank_supported(6040, 3706, 128, 64)
    assert not tr.target_rank_supported(10, 10, 20, 1) and not tr.target_rank_supported(10, 10, 64, 65) and not tr.target_rank_supported(10, 10, 64, 0)
    assert not tr.target_rank_supported(tr.TARGETRANK_MAX_ROWS + 1, 10, 64, 1) and not tr.target_rank_supported(10, tr.TARGETRANK_MAX_ROWS + 1, 64, 1)
    assert not tr.target_rank_supported(10, 10, 64, 1, 2 ** 31) and not tr.target_rank_supported(0, 10, 64, 1)


def test_dispatcher_takes_the_composed_route_for_cpu_tensors_and_past_the_limits():
    from arlib_amd import targetrank as tr, ops
    assert ops.target_rank is tr.target_rank and ops.target_rank_kernel is tr.target_rank_kernel and ops.target_rank_composed is tr.target_rank_composed
    Pu, Pi, targets, mask, ref = case(1, True)
    rank, _ = tr.target_rank(tens(Pu), tens(Pi), tens(targets), (tens(mask[0]), tens(mask[1])))
    assert R.check_bracket(rank.numpy(), ref) == []
    rng = np.random.default_rng(5)
    Pu, Pi = rng.standard_normal((9, 20)).astype(np.float32), rng.standard_normal((70, 20)).astype(np.float32)          # d = 20 and T = 65
    targets = rng.choice(70, 65, replace=False).astype(np.int32)
    rank, _ = tr.target_rank(tens(Pu), tens(Pi), tens(targets))
    assert R.check_bracket(rank.numpy(), R.restate(Pu, Pi, targets)) == []


def test_header_exports_and_argument_checks():
    from arlib_amd import _lib, targetrank as tr
    assert _lib.ABI_VERSION == 34
    names = ('arl_target_rank_workspace_bytes', 'arl_target_rank_f32')
    hdr = open(os.path.join(ROOT, 'include', 'arlib_amd.h')).read()
    for name in names:
        assert name in _lib.EXPORTS and re.search(r'/\* util/metrics\.py:125-208 \*/\n[^\n]*\b%s\s*\(' % name, hdr), name
    L = _lib.lib()
    assert L.arl_abi_version() == 34
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    big = tr.TARGETRANK_MAX_ROWS + 1
    f = L.arl_target_rank_f32                                  # arguments are checked before any launch: no device is needed to be told so
    assert f(None, 4, p, 4, 16, p, 1, None, None, p, p, p, None) == -1
    assert f(p, 4, p, 4, 16, None, 1, None, None, p, p, p, None) == -1
    assert f(p, 4, p, 4, 16, p, 1, None, None, p, p, None, None) == -1
    assert f(p, 4, p, 4, 16, p, 1, p, None, p, p, p, None) == -1                    # a missing mask half
    assert f(p, 4, p, 4, 16, p, 1, None, p, p, p, p, None) == -1
    assert f(p, 4, p, 4, 20, p, 1, None, None, p, p, p, None) == -3                 # d = 20
    assert f(p, 4, p, 4, 16, p, 65, None, None, p, p, p, None) == -3                # T = 65
    assert f(p, 4, p, 4, 16, p, 0, None, None, p, p, p, None) == -3                 # T = 0
    assert f(p, big, p, 4, 16, p, 1, None, None, p, p, p, None) == -3
    assert f(p, 4, p, big, 16, p, 1, None, None, p, p, p, None) == -3
    assert f(p, 0, p, 4, 16, p, 1, None, None, p, p, p, None) == -3
    assert f(p + 4, 4, p, 4, 16, p, 1, None, None, p, p, p, None) == -4
    w = L.arl_target_rank_workspace_bytes
    assert w(10, 10, 20, 1) == 0 and w(10, 10, 16, 65) == 0 and w(0, 10, 16, 1) == 0
    assert w(1_000_000, 100_000, 64, 64) == 0                                       # a long user side: the stream is not split, the counts go to `rank`
    assert w(65, 4097, 64, 64) % 16 == 0 and w(65, 4097, 64, 64) >= 2 * 4 * 65 * 64     # a short one: integer partials per split

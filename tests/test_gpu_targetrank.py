"""The target-rank kernel (csrc/arl_targetrank.hip) on the GPU against the float64 restatement of tests/rank_restatement.py: every fixed case, masked
and unmasked, must lie in the bracket [lo, hi] that the fp32 rounding bound allows (at most 2 wide on these cases, test_targetrank_cpu.py), be exact
on integer tables and put -1 exactly where the target is listed; the calls are bit-identical; the dispatcher, the composed route on the device and
util.metrics.TargetRankMetric are held to the same restatement."""
import numpy as np
import pytest
import torch
import rank_restatement as R
from test_targetrank_cpu import case, tens, StubModel, hold_metric

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ALL = range(len(R.CASES))


def run(fn, k, masked, integer=False):
    Pu, Pi, targets, mask, ref = case(k, masked, integer)
    rank, ts = fn(tens(Pu, DEV), tens(Pi, DEV), tens(targets, DEV), (tens(mask[0], DEV), tens(mask[1], DEV)) if masked else None)
    assert rank.dtype == torch.int32 and ts.dtype == torch.float32 and rank.shape == ts.shape == (Pu.shape[0], len(targets)) and rank.is_cuda
    return rank, ts, ref


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', ALL, ids=R.IDS)
def test_kernel_lies_in_the_bracket(k, masked):
    from arlib_amd import ops
    rank, ts, ref = run(ops.target_rank_kernel, k, masked)
    rank, ts = rank.cpu().numpy(), ts.cpu().numpy()
    gap = (ref['hi'] - ref['lo'])[~ref['listed']]
    print('%s masked %d: %d of %d valid pairs differ from the float64 rank, bracket at most %d wide' %
          (R.IDS[k], masked, int((rank != ref['rank0'])[~ref['listed']].sum()), gap.size, gap.max() if gap.size else 0))
    assert R.check_bracket(rank, ref) == []
    assert (np.abs(ts.astype(np.float64) - ref['tscore']) <= ref['tbound']).all()


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', ALL, ids=R.IDS)
def test_kernel_is_exact_on_integer_tables(k, masked):
    from arlib_amd import ops
    rank, ts, ref = run(ops.target_rank_kernel, k, masked, integer=True)
    rank = rank.cpu().numpy()
    assert np.array_equal(rank, ref['rank0']), '%d pairs differ' % int((rank != ref['rank0']).sum())
    assert np.array_equal(rank == -1, ref['listed'])
    assert np.array_equal(ts.cpu().numpy().astype(np.float64), ref['tscore'])


@pytest.mark.parametrize('k', [2, 4], ids=[R.IDS[2], R.IDS[4]])
def test_two_calls_give_identical_bits(k):
    from arlib_amd import ops
    for integer in (False, True):
        a = run(ops.target_rank_kernel, k, True, integer)
        b = run(ops.target_rank_kernel, k, True, integer)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', ALL, ids=R.IDS)
def test_kernel_and_composed_differ_only_inside_the_bracket(k, masked):
    from arlib_amd import ops
    rank, ts, ref = run(ops.target_rank_kernel, k, masked)
    crank, cts, _ = run(ops.target_rank_composed, k, masked)
    rank, crank = rank.cpu().numpy().astype(np.int64), crank.cpu().numpy().astype(np.int64)
    assert R.check_bracket(crank, ref) == []
    d = rank != crank
    assert not (d & ref['listed']).any()
    for r in (rank, crank):
        assert ((ref['lo'] <= r) & (r <= ref['hi']))[d].all()
    assert (np.abs(ts.cpu().numpy().astype(np.float64) - cts.cpu().numpy()) <= 2 * ref['tbound']).all()
    irank, _, iref = run(ops.target_rank_composed, k, masked, integer=True)
    assert np.array_equal(irank.cpu().numpy(), iref['rank0'])


def test_dispatcher_takes_the_kernel_inside_the_limits_and_the_composed_route_past_them(monkeypatch):
    from arlib_amd import targetrank as tr
    taken = []
    kernel, comp = tr.target_rank_kernel, tr.target_rank_composed
    monkeypatch.setattr(tr, 'target_rank_kernel', lambda *a, **kw: (taken.append('kernel'), kernel(*a, **kw))[1])
    monkeypatch.setattr(tr, 'target_rank_composed', lambda *a, **kw: (taken.append('composed'), comp(*a, **kw))[1])
    rank, _, ref = run(tr.target_rank, 1, True)
    assert taken == ['kernel'] and R.check_bracket(rank.cpu().numpy(), ref) == []
    rng = np.random.default_rng(5)
    for U, I, d, T in ((9, 70, 20, 3), (9, 70, 16, 65)):                             # d = 20; T = 65
        Pu, Pi = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
        targets = rng.choice(I, T, replace=False).astype(np.int32)
        mask = R.draw_mask(U, I, targets, 7)
        del taken[:]
        rank, _ = tr.target_rank(tens(Pu, DEV), tens(Pi, DEV), tens(targets, DEV), (tens(mask[0], DEV), tens(mask[1], DEV)))
        assert taken == ['composed'] and R.check_bracket(rank.cpu().numpy(), R.restate(Pu, Pi, targets, mask)) == []
        with pytest.raises(ValueError):
            kernel(tens(Pu, DEV), tens(Pi, DEV), tens(targets, DEV))


@pytest.mark.parametrize('integer', [False, True], ids=['normal', 'integer'])
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
def test_metric_on_a_gpu_model_lies_in_the_float64_intervals(masked, integer):
    from arlib_amd.util.metrics import TargetRankMetric
    k = 5
    Pu, Pi, targets, _, ref = case(k, masked, integer)
    mask = R.draw_mask(Pu.shape[0], Pi.shape[0], targets, R.CASES[k][4])
    ks = [1, 10, 50, 129, 500, Pi.shape[0]]                                          # 129 and up: past what a top-k list of score_mask_topk reaches
    metric = TargetRankMetric(StubModel(Pu, Pi, mask, DEV), targets.tolist(), top=ks, mask_train=masked)
    hold_metric(metric, ref, ks, integer)


def test_metric_agrees_with_attack_metric_on_integer_tables_without_ties_at_the_cut():
    """The four reference numbers from the rank matrix are AttackMetric's own where its top-k list is unambiguous: unmasked, and a k whose cut does not
    fall inside a group of tied scores for any user (checked in float64 below)."""
    from arlib_amd.util.metrics import TargetRankMetric, AttackMetric
    Pu, Pi, targets, _, ref = case(1, False)
    S = np.sort(Pu.astype(np.float64) @ Pi.astype(np.float64).T, axis=1)[:, ::-1]
    ks = [k for k in (5, 10, 50) if (S[:, k - 1] - S[:, k] > 1e-4).all()]
    assert ks
    model = StubModel(Pu, Pi, R.draw_mask(Pu.shape[0], Pi.shape[0], targets, 1), DEV)
    a, b = AttackMetric(model, targets.tolist(), top=ks), TargetRankMetric(model, targets.tolist(), top=ks)
    for name in ('hitRate', 'precision', 'recall', 'NDCG'):
        assert np.allclose(getattr(a, name)(), getattr(b, name)(), rtol=0, atol=1e-12), name


def test_arguments_are_refused_as_by_the_other_ops():
    from arlib_amd import ops
    from arlib_amd._lib import ArlError
    Pu, Pi, targets, mask, _ = case(1, True)
    g = lambda a: tens(a, DEV)
    with pytest.raises(ArlError):
        ops.target_rank_kernel(tens(Pu), g(Pi), g(targets))                          # a table in host memory
    with pytest.raises(ArlError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(targets), (tens(mask[0]), g(mask[1])))
    with pytest.raises(ValueError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(targets), (g(mask[0]), None))         # a missing mask half
    with pytest.raises(ValueError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(targets), (None, g(mask[1])))
    with pytest.raises(IndexError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(np.array([3, 3], np.int32)))
    with pytest.raises(IndexError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(np.array([Pi.shape[0]], np.int32)))
    bad = mask[0].copy(); bad[3] = bad[2] - 1
    with pytest.raises(IndexError):
        ops.target_rank_kernel(g(Pu), g(Pi), g(targets), (g(bad), g(mask[1])))

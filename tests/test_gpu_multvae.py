"""Mult-VAE / Mult-DAE on the device, on a util/synthetic set of 300 users and 200 items: three training steps on the kernel route and on the composed
route against the float64 restatement (tests/multvae_restatement.py) fed the same (rows, keep, eps); training lowers the likelihood; the exposed
tables are the model's ranking; and the attack flow (RandomAttack, retraining on the poisoned data, AttackMetric and TargetRankMetric) runs through
_base.Recommender unchanged.

Bar for the weights after three steps: the project's own (test_gpu_multinomial.py) -- the max-norm relative error against float64 is at most
FACTOR = 4 times the composed fp32 route's error on the same steps, with FLOOR = 1e-6."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import multvae_restatement as R
from test_multvae_cpu import synthetic_data, fresh, batches_for, dense_profiles_of, rec_args, rel
from test_gpu_attack_edges import topk_ref64, check_near_ties

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FACTOR, FLOOR = 4.0, 1e-6
NAMES = ('W_enc', 'b_enc', 'W_dec')


@pytest.fixture(scope='module')
def data():
    return synthetic_data()


def run_steps(rec, batches, lr=0.01):
    rec.model.cuda()
    opt = torch.optim.Adam(rec._params(), lr=lr)
    losses = [rec.step(rows, keep, eps, opt)[0] for rows, keep, eps in batches]
    return [p.detach().cpu() for p in rec._params()], [float(l) for l in losses]


@pytest.mark.parametrize('variational', [True, False], ids=['vae', 'dae'])
def test_three_steps_on_both_routes_against_float64(data, variational):
    recs = {route: fresh(data, vae_variational=variational, vae_route=route) for route in ('fused', 'composed')}
    W0 = [p.detach().clone() for p in recs['fused']._params()]
    assert all(torch.equal(a, b.detach()) for a, b in zip(W0, recs['composed']._params()))
    X = dense_profiles_of(recs['fused'])
    batches = batches_for(recs['fused'], 3)
    want, outs = R.train_steps(*W0, X, batches, lr=0.01, vae_beta=0.5, anneal_steps=2, reg=1e-3, dropout=0.5, variational=variational)
    got = {route: run_steps(rec, batches) for route, rec in recs.items()}
    for route in got:
        for t, r in enumerate(outs):
            assert abs(got[route][1][t] - float(r['loss'])) <= 1e-5 * float(r['loss']), (route, t)
    for k, name in enumerate(NAMES):
        ek, ec = rel(got['fused'][0][k], want[k]), rel(got['composed'][0][k], want[k])
        print('multvae %s three steps %s: kernel route %.3e composed route %.3e' % ('vae' if variational else 'dae', name, ek, ec))
        assert ek <= max(FACTOR * ec, FLOOR), (name, ek, ec)
        assert float((got['fused'][0][k] - W0[k]).abs().max()) > 0.01          # the steps moved the weights (3 Adam steps of lr 0.01)


@pytest.mark.parametrize('route', ['fused', 'auto'])
def test_twenty_steps_lower_the_training_nll(data, route):
    rec = fresh(data, vae_route=route, vae_batch_users=128)
    m = rec.model.cuda()
    rows = torch.arange(data.user_num)
    nnz = int(m.rowptr[-1])

    def nll():
        with torch.no_grad():                                        # the whole table, no dropout, no sampling
            return float(m.step_loss(rows, torch.ones(nnz, dtype=torch.bool), torch.zeros(data.user_num, 16), 0.0, 0.0, 0.0, route)[1])
    before = nll()
    opt = torch.optim.Adam(rec._params(), lr=0.01)
    for rows_b, keep, eps in batches_for(rec, 20, seed=11):
        rec.step(rows_b, keep, eps, opt)
    after = nll()
    print('multvae twenty steps (%s): nll %.4f -> %.4f' % (route, before, after))
    assert np.isfinite(after) and after < before - 0.05 and rec.steps_done == 20


def test_trained_tables_are_the_ranking(data):
    rec = fresh(data, vae_route='fused', maxEpoch=2)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rec.train(evalNum=1)
        rec_list, measure = rec.test()
    assert 'training: 1 batch 0 nll: ' in buf.getvalue() and rec.steps_done == 2 * ((data.user_num + 63) // 64)
    assert measure[0] == 'Top 10\n' and any(m.startswith('Recall:') for m in measure) and len(rec_list) == len(data.test_set)
    rec.save()
    ue, ie = rec.model()
    assert rec.best_user_emb.is_cuda and torch.equal(rec.best_user_emb, ue) and torch.equal(rec.best_item_emb, ie.detach())
    # user_emb is mu of a fresh whole-table encode: float64, no dropout, no sampling
    Xd = dense_profiles_of(rec).double()
    W, b = rec.model.embedding_dict['W_enc'].detach().cpu().double(), rec.model.embedding_dict['b_enc'].detach().cpu().double()
    mu = (Xd / Xd.sum(1, keepdim=True).sqrt()) @ W[:, :16] + b[:16]
    assert rel(ue.cpu(), mu) <= 2e-6
    # test()'s lists are torch.topk(user_emb @ item_emb.T) with the training items masked, up to near-ties
    rec.user_emb, rec.item_emb = ue, ie.detach()
    users, idx, val = rec._test_topk()
    uid = [data.user[u] for u in users]
    cols = [np.sort(np.fromiter((data.item[it] for it in data.training_set_u[u]), dtype=np.int32)) for u in users]
    ridx, rval = topk_ref64(ue[uid], ie.detach(), 10, cols)
    check_near_ties(torch.from_numpy(idx).to(DEV).to(torch.int32), torch.from_numpy(val).to(DEV), ridx, rval)
    assert np.allclose(rec.predict(users[0]), (ue[uid[0]] @ ie.detach().T).cpu().numpy(), rtol=0, atol=1e-5)


def test_random_attack_flow_and_both_metric_classes(data, tmp_path, monkeypatch):
    from arlib_amd.util.tool import seedSet, dataSave
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.FileIO import FileIO
    from arlib_amd.util.metrics import AttackMetric, TargetRankMetric
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    from types import SimpleNamespace
    monkeypatch.chdir(tmp_path)
    seedSet(2018)
    rec = fresh(data, maxEpoch=2)
    atk = RandomAttack(SimpleNamespace(maliciousUserSize=0.05, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular',
                                       targetSize=5), data)
    poison = atk.posionDataAttack()
    out_dir = 'data/poison/RandomAttack_syn/0/'
    os.makedirs(out_dir, exist_ok=True)
    dataSave(poison, out_dir + 'train.txt', data.id2user, data.id2item)
    FileIO.write_file(out_dir, 'test.txt', ['%s %s %s\n' % (u, i, r) for u, i, r in data.test_data])
    FileIO.write_file(out_dir, 'val.txt', [])
    pargs = rec_args(dataset='RandomAttack_syn/0', data_path='data/poison/', training_data='/train.txt', val_data='/val.txt', test_data='/test.txt', maxEpoch=2)
    pdata = DataLoader(pargs)
    U, F = data.user_num, atk.fakeUserNum
    assert F > 0 and pdata.user_num == U + F and pdata.item_num == data.item_num
    with contextlib.redirect_stdout(io.StringIO()):
        rec.__init__(pargs, pdata)                                       # the driver's order: same object, poisoned data
        rec.train(evalNum=1)
        _, after = rec.test()
    assert after[0] == 'Top 10\n' and rec.user_emb.shape == (U + F, 16) and rec.model.embedding_dict['W_enc'].shape == (data.item_num, 32)
    a, b = AttackMetric(rec, atk.targetItem, [10]), TargetRankMetric(rec, atk.targetItem, [10])
    # the two classes agree except on a (user, target) pair whose score is within 1e-4 of the user's cut (its 10th and 11th scores) in float64
    S = rec.user_emb.double() @ rec.item_emb.double().T
    top = torch.sort(S, dim=1, descending=True)[0]
    T = S[:, torch.tensor([int(t) for t in atk.targetItem], device=S.device)]
    amb = int((((T - top[:, 9:10]).abs() < 1e-4) | ((T - top[:, 10:11]).abs() < 1e-4)).sum())
    n_u, n_t = S.shape[0], len(atk.targetItem)
    print('multvae attack flow: hitRate %.5f / %.5f, %d ambiguous pairs' % (a.hitRate()[0], b.hitRate()[0], amb))
    assert abs(a.hitRate()[0] - b.hitRate()[0]) <= amb / (n_u * n_t) + 1e-12
    assert abs(a.recall()[0] - b.recall()[0]) <= amb / (n_u * n_t) + 1e-12
    assert abs(a.precision()[0] - b.precision()[0]) <= amb / (n_u * 10) + 1e-12
    assert 0.0 <= b.hitRate()[0] <= 1.0 and b.meanRank() >= 1.0

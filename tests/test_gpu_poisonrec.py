"""PoisonRec and RLAttack on the device with a real LightGCN (d 16) on a 300 x 120 synthetic data set, F = 4, Epoch = 1 retrains: the first policy
update's gradients on the fused route against the float64 restatement (tests/poisonrec_restatement.py) with the composed route as the yardstick,
the fused attack's run-to-run determinism and fake-row contract, and RLAttack end to end.

Whole fused and composed attacks are not compared sample for sample: fp32 rounding may flip a borderline draw after the first update.  The
first-update gradient check is the comparison that means something.  Bar: test_gpu_policyhead.py's FACTOR = 4 and FLOOR = 1e-6."""
import contextlib
import copy
import io

import numpy as np
import pytest
import scipy.sparse as sp
import torch
from test_gpu_api import rec_args
from test_gpu_policyhead import held
from test_shilling_cpu import attack_args
import poisonrec_restatement as rs

pytestmark = pytest.mark.gpu
U, I, F, K, T = 300, 120, 4, 6, 2


def problem(name, seed=2018, **kw):
    """A fresh data set, a LightGCN trained for one epoch on it, and the attack."""
    import importlib
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.LightGCN import LightGCN
    rng = np.random.default_rng(5)
    train = set((u, int(i)) for u in range(U) for i in rng.choice(I, 8, replace=False))
    train |= set((int(rng.integers(U)), i) for i in range(I))
    test = set((u, int(rng.integers(I))) for u in range(0, U, 3)) - train
    tr, te = np.array(sorted(train)), np.array(sorted(test))
    ones = lambda a: np.ones(len(a), np.float32)
    data = DataLoader.from_arrays((tr[:, 0], tr[:, 1], ones(tr)), (te[:, 0], te[:, 1], ones(te)), (te[:, 0], te[:, 1], ones(te)), dataName='poisonrec-syn',
                                  array_native=False)
    assert (data.user_num, data.item_num) == (U, I)
    seedSet(seed)
    rec = LightGCN(rec_args(emb_size=16, n_layers=2, maxEpoch=1), data)
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train(Epoch=1, evalNum=5)
    cls = getattr(importlib.import_module('arlib_amd.attack.Black.' + name), name)
    atk = cls(attack_args(name, 'Black', maliciousUserSize=F, maliciousFeedbackSize=K, targetSize=T), data, **kw)
    atk.retrain_epochs = 1
    return atk, rec, data


def test_first_policy_update_gradients_against_float64():
    from arlib_amd.attack.Black import _ppo
    from arlib_amd.util.tool import seedSet
    atk, rec, _ = problem('PoisonRec', dim=16)
    assert atk.policy_route == 'fused' and atk.noise_source == 'torch'
    seedSet(7)
    with contextlib.redirect_stdout(io.StringIO()):
        atk.fakeUserInject(rec)
        atk._build(rec)
        ppo = atk.agent
        ppo.collect_rollout()
    buf, pol = ppo.buffer, ppo.policy
    assert buf.rewards[:F - 1] == [0.0] * (F - 1) and np.isfinite(buf.rewards[-1]) and buf.actions.shape == (F, (I + 31) // 32)
    rows = np.arange(F)
    users, offsets, idx = buf.observations(rows)
    names = [n for n, _ in pol.named_parameters()]
    t32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32, device='cuda')

    def device_grads(route):
        pol.route = route
        values, logp, ent = pol.evaluate(users, offsets, idx, buf.actions)
        loss, kl = _ppo.ppo_minibatch_loss(logp, t32(buf.logps), ent, values, t32(buf.advantages), t32(buf.returns), ppo.clip_range, ppo.ent_coef, ppo.vf_coef)
        return loss.detach(), kl, torch.autograd.grad(loss, list(pol.parameters()), allow_unused=True)
    loss_f, kl_f, g_f = device_grads('fused')
    loss_c, kl_c, g_c = device_grads('composed')
    pol.route = 'fused'
    pol64 = copy.deepcopy(pol).cpu().double()
    profiles = [buf.idx[buf.ptr[r]:buf.ptr[r + 1]] for r in rows]
    t64 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    loss64, kl64 = rs.policy_loss(pol64, users, profiles, rs.unpack(buf.actions, I), t64(buf.logps), t64(buf.advantages), t64(buf.returns), ppo.clip_range,
                                  ppo.ent_coef, ppo.vf_coef)
    g64 = torch.autograd.grad(loss64, list(pol64.parameters()), allow_unused=True)
    print('first update: loss fused %.8f composed %.8f float64 %.8f; KL %.3e %.3e %.3e' % (float(loss_f), float(loss_c), float(loss64), kl_f, kl_c, kl64))
    assert abs(float(loss_f) - float(loss64)) <= 1e-4 * max(1.0, abs(float(loss64))) and kl_f < 1e-6
    checked = 0
    for name, a, b, w in zip(names, g_f, g_c, g64):
        assert (a is None) == (b is None) == (w is None), name
        if w is not None and float(w.abs().max()) > 0:
            held('first update', name, a, b, w)
            checked += 1
    assert checked >= 12                                                  # both embeddings, the LSTM's 8 tensors, the DNN's 4, the value net's


def fused_attack(seed, noise):
    atk, rec, data = problem('PoisonRec', dim=16)
    atk.seed, atk.total_timesteps, atk.noise_source = seed, 2 * F, noise
    before = sp.csr_matrix(atk.interact).copy()
    with contextlib.redirect_stdout(io.StringIO()):
        res = sp.csr_matrix(atk.posionDataAttack(rec))
    return atk, rec, before, res


@pytest.mark.parametrize('noise', ['torch', 'hash'])
def test_fused_attack_contract_and_determinism(noise):
    from arlib_amd.util.metrics import AttackMetric
    atk, rec, before, res = fused_attack(11, noise)
    assert atk.policy_route == 'fused' and atk.agent.policy.route == 'fused' and atk.noise_source == noise
    assert atk.agent.num_timesteps == 2 * F and atk.agent.n_rollouts == 2 and len(atk.agent.reward_stats) == 2
    assert res.shape == (U + F, I) == atk.interact.shape and (res[:U] != before).nnz == 0
    fake = np.asarray(res[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0} and (fake[:, atk.targetItem] == 1).all()
    assert ((fake.sum(1) >= K) & (fake.sum(1) <= K + T)).all() and atk.fakeUser == list(range(U, U + F))
    hit = AttackMetric(rec, atk.targetItem, [50]).hitRate()[0]
    assert np.isfinite(hit) and 0.0 <= hit <= 1.0
    atk2, _, _, res2 = fused_attack(11, noise)
    assert (res != res2).nnz == 0                                         # bit-identical from run to run
    assert all(torch.equal(a, b) for a, b in zip(atk.agent.policy.parameters(), atk2.agent.policy.parameters()))
    assert atk.agent.update_log == atk2.agent.update_log and atk.agent.reward_stats == atk2.agent.reward_stats


def test_rlattack_end_to_end():
    def run():
        atk, rec, data = problem('RLAttack')
        atk.seed, atk.total_timesteps = 3, 8
        before = sp.csr_matrix(atk.interact).copy()
        with contextlib.redirect_stdout(io.StringIO()):
            res = sp.csr_matrix(atk.posionDataAttack(rec))
        return atk, before, res
    atk, before, res = run()
    assert res.shape == (U + F, I) and (res[:U] != before).nnz == 0 and atk.agent.num_timesteps == 20
    fake = np.asarray(res[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0} and (fake[:, atk.targetItem] == 1).all() and (fake.sum(1) <= K + T).all()
    assert all(r > 0 or r == 0 for r in atk.agent.buffer.rewards) and np.isfinite(atk.agent.buffer.rewards).all()
    _, _, res2 = run()
    assert (res != res2).nnz == 0

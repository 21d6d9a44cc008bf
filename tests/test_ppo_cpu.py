"""The PPO of PoisonRec and RLAttack (arlib_amd/attack/Black/_ppo.py) without a GPU, in float64 against the restatement
(tests/poisonrec_restatement.py) to 1e-12: GAE over episode boundaries, the clipped update with its minibatch permutations, its KL stop firing in
the second epoch and the gradient-norm clip, and the entropy-coefficient schedule."""
import copy

import numpy as np
import pytest
import torch
import poisonrec_restatement as rs


class ToyEnv:
    """Episodes of `length` steps over `I` items; the observation is (0, the action's item ids), the reward a fixed function of the action."""

    def __init__(self, I, length=5):
        self.I, self.length, self.t = I, length, 0
        self.w = np.cos(np.arange(I))

    def reset(self):
        self.t = 0
        return 0, np.array([0], np.int64)

    def step(self, action):
        self.t += 1
        items = np.where(action == 1)[0]
        return (0, items if len(items) else np.array([0], np.int64)), float(self.w @ action), self.t == self.length


def toy_ppo(I=12, **kw):
    from arlib_amd.attack.Black import _ppo
    torch.manual_seed(3)
    policy = _ppo.MlpBernoulliPolicy(I).double()
    args = dict(learning_rate=0.05, n_steps=12, batch_size=6, n_epochs=4, gamma=0.9, gae_lambda=0.95, clip_range=0.1, ent_coef=0.1, vf_coef=0.5,
                max_grad_norm=0.5, target_kl=None)
    args.update(kw)
    return _ppo.PPO(policy, ToyEnv(I), **args)


@pytest.mark.parametrize('last_done', [0.0, 1.0])
def test_gae_against_the_restatement(last_done):
    from arlib_amd.attack.Black import _ppo
    rng = np.random.default_rng(4)
    n = 23
    rewards, values = rng.normal(size=n), rng.normal(size=n)
    starts = (rng.random(n) < 0.25).astype(np.float64)
    starts[0] = 1.0
    for gamma, lam in ((1.0, 0.95), (0.9, 0.8)):
        adv, ret = _ppo.gae(rewards, values, starts, 0.7, last_done, gamma, lam)
        adv64, ret64 = rs.gae(rewards, values, starts, 0.7, last_done, gamma, lam)
        assert np.abs(adv - adv64).max() <= 1e-12 and np.abs(ret - ret64).max() <= 1e-12
    # PoisonRec's rollout: one episode, gamma 1, the reward at the last step only, the bootstrap value dropped
    r = np.zeros(6); r[-1] = 3.0
    v = rng.normal(size=6)
    adv, ret = _ppo.gae(r, v, [1, 0, 0, 0, 0, 0], 9.9, 1.0, 1.0, 0.95)
    assert abs(ret[-1] - 3.0) <= 1e-12 and abs(adv[-1] - (3.0 - v[-1])) <= 1e-12


def restated_update(ppo, policy, optimizer, rng_state):
    """The update of ppo.train() on a copy of the policy, from the restatement's loss and the same permutations."""
    buf = ppo.buffer
    n = len(buf.rewards)
    adv, ret, old = (torch.as_tensor(np.asarray(x), dtype=torch.float64) for x in (buf.advantages, buf.returns, buf.logps))
    np.random.set_state(rng_state)
    log = dict(epochs=0, steps=0, stopped=False, kl=[])
    for epoch in range(ppo.n_epochs):
        order = np.random.permutation(n)
        for lo in range(0, n, ppo.batch_size):
            rows = order[lo:lo + ppo.batch_size]
            users, offsets, idx = buf.observations(rows)
            values, logp, ent = policy.evaluate(users, offsets, idx, buf.actions[torch.as_tensor(rows)])
            sel = torch.as_tensor(rows)
            loss, kl = rs.ppo_loss(logp, old[sel], ent, values, adv[sel], ret[sel], ppo.clip_range, ppo.ent_coef, ppo.vf_coef)
            log['kl'].append(kl)
            if ppo.target_kl is not None and kl > 1.5 * ppo.target_kl:
                log['stopped'] = True
                return log
            optimizer.zero_grad()
            loss.backward()
            total = torch.sqrt(sum((p.grad ** 2).sum() for p in policy.parameters()))
            coef = ppo.max_grad_norm / (float(total) + 1e-6)                 # torch's clip_grad_norm_
            if coef < 1:
                for p in policy.parameters():
                    p.grad.mul_(coef)
            optimizer.step()
            log['steps'] += 1
        log['epochs'] += 1
    return log


@pytest.mark.parametrize('target_kl,batch_size', [(None, 6), (0.002, 12)])
def test_update_against_the_restatement(target_kl, batch_size):
    ppo = toy_ppo(target_kl=target_kl, batch_size=batch_size)
    np.random.seed(5)
    ppo.collect_rollout()
    assert len(ppo.buffer.rewards) == 12 and ppo.buffer.actions.shape == (12, 1) and ppo.buffer.actions.dtype == torch.int32
    assert ppo.buffer.starts == [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    twin = copy.deepcopy(ppo.policy)
    twin_opt = torch.optim.Adam(twin.parameters(), lr=0.05, eps=1e-5)
    state = np.random.get_state()
    log = ppo.train()
    want = restated_update(ppo, twin, twin_opt, state)
    print('update target_kl=%s: %s' % (target_kl, {k: log[k] for k in ('epochs', 'steps', 'stopped')}), log['kl'])
    assert (log['epochs'], log['steps'], log['stopped']) == (want['epochs'], want['steps'], want['stopped'])
    assert np.abs(np.array(log['kl']) - np.array(want['kl'])).max() <= 1e-12
    for a, b in zip(ppo.policy.parameters(), twin.parameters()):
        assert float((a - b).detach().abs().max()) <= 1e-12 * max(1.0, float(b.detach().abs().max()))
    if target_kl is None:
        assert (log['epochs'], log['steps'], log['stopped']) == (4, 8, False)
    else:
        # one minibatch per epoch: the first is stepped at ratio 1 (KL 0 up to rounding); the second epoch's exceeds 1.5 * target_kl, is not
        # stepped, and the remaining epochs are dropped
        assert log['stopped'] and (log['epochs'], log['steps'], len(log['kl'])) == (1, 1, 2)
        assert log['kl'][0] < 1e-20 and log['kl'][1] > 1.5 * target_kl


def test_entropy_coefficient_schedule_and_reward_statistics():
    ppo = toy_ppo(n_steps=50, batch_size=50, n_epochs=1, ent_decay_every=100, ent_decay=0.9, log_reward_stats=True)
    np.random.seed(6)
    ppo.learn(total_timesteps=250)
    assert ppo.num_timesteps == 250 and ppo.n_rollouts == 5
    assert abs(ppo.ent_coef - 0.1 * 0.9 ** 2) <= 1e-15                                      # multiplied at timesteps 100 and 200
    assert len(ppo.reward_stats) == 5 and all(s[1] > 0 and s[2] < 0 < s[3] for s in ppo.reward_stats)
    # the statistics are recorded after the returns exist and the buffer is left alone: returns - advantages are still the values
    buf = ppo.buffer
    assert np.abs(buf.returns - buf.advantages - np.array(buf.values)).max() <= 1e-12
    assert np.abs(np.array(buf.rewards)).max() > 1.5                                        # not normalised in place

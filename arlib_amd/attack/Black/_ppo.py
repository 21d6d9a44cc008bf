"""What PoisonRec and RLAttack take from stable_baselines3 and gym, written out: a rollout buffer with GAE, the clipped PPO update with its KL stop
and gradient-norm clip, the two callbacks' effects, the two policies and the two environments.  No gym, no stable_baselines3; CPU and GPU.

PPO as stable_baselines3 runs it with the reference's arguments: Adam(lr, eps=1e-5); per rollout n_steps environment steps, then n_epochs passes
over the buffer in minibatches drawn from one np.random.permutation per pass (the global numpy generator, as SB3's buffer does); advantages
normalised per minibatch as (A - mean) / (std + 1e-8); loss = policy + ent_coef * (-mean entropy) + vf_coef * MSE(returns, values) with
policy = -mean min(r A, clip(r, 1 +- clip_range) A); a minibatch whose approximate KL mean((r - 1) - log r) exceeds 1.5 * target_kl is not stepped
and ends the update; gradients are clipped to max_grad_norm.  GAE: delta_t = r_t + gamma V_(t+1) (1 - start_(t+1)) - V_t, the value after an
episode's last step is 0.

Buffer layout: observations are index lists (user id, CSR over the rollout of the profile's item ids), actions are packed bits
(ops.pack_bits: [n, ceil(I / 32)] int32); no n x I tensor is kept."""
import contextlib
import io
import random

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
import torch.nn.functional as Fn

from ... import policyhead
from ...util.metrics import AttackMetric
from .._common import init_graph, rebuild_interaction_matrix, append_rows


# ------------------------------------------------------------------------------------------------ GAE, loss, buffer
def gae(rewards, values, episode_starts, last_value, last_done, gamma, gae_lambda):
    """(advantages, returns) in float64 for one rollout.  episode_starts[t] = 1 when step t began an episode; last_done = 1 when the rollout's last
    step ended one, which drops the bootstrap value last_value."""
    rewards, values, starts = (np.asarray(x, np.float64) for x in (rewards, values, episode_starts))
    n = len(rewards)
    adv = np.zeros(n, np.float64)
    last = 0.0
    for t in range(n - 1, -1, -1):
        nonterminal = 1.0 - (float(last_done) if t == n - 1 else starts[t + 1])
        next_value = float(last_value) if t == n - 1 else values[t + 1]
        delta = rewards[t] + gamma * next_value * nonterminal - values[t]
        last = delta + gamma * gae_lambda * nonterminal * last
        adv[t] = last
    return adv, adv + values


def ppo_minibatch_loss(logp_new, logp_old, ent, values, adv, returns, clip_range, ent_coef, vf_coef):
    """(loss, approximate KL as a float) of one minibatch."""
    if adv.numel() > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    log_ratio = logp_new - logp_old
    ratio = torch.exp(log_ratio)
    policy = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip_range, 1 + clip_range) * adv).mean()
    value = Fn.mse_loss(returns, values)
    loss = policy + ent_coef * (-ent.mean()) + vf_coef * value
    with torch.no_grad():
        kl = float(((ratio - 1) - log_ratio).mean())
    return loss, kl


class RolloutBuffer:
    """n_steps transitions.  Observations: users [n] and the CSR (ptr [n + 1], idx) of the profiles' item ids; actions: packed words [n, W]."""

    def __init__(self, n_steps):
        self.n_steps = int(n_steps)
        self.reset()

    def reset(self):
        self.users, self.ptr, self._idx, self.idx = [], [0], [], None
        self.actions, self.rewards, self.starts, self.values, self.logps = [], [], [], [], []
        self.advantages = self.returns = None

    def add(self, obs, action_words, reward, episode_start, value, logp):
        user, items = obs
        items = np.asarray(items, np.int64)
        self.users.append(int(user)); self._idx.append(items); self.ptr.append(self.ptr[-1] + len(items))
        self.actions.append(action_words.reshape(1, -1)); self.rewards.append(float(reward)); self.starts.append(float(episode_start))
        self.values.append(float(value)); self.logps.append(float(logp))

    def finish(self, last_value, last_done, gamma, gae_lambda):
        self.idx = np.concatenate(self._idx) if self._idx else np.zeros(0, np.int64)
        self.actions = torch.cat(self.actions, 0)
        self.advantages, self.returns = gae(self.rewards, self.values, self.starts, last_value, last_done, gamma, gae_lambda)

    def observations(self, rows):
        """(users, offsets, idx) of the buffer rows `rows`: the index-list batch a policy's evaluate() takes."""
        ptr = np.asarray(self.ptr, np.int64)
        lens = ptr[1:][rows] - ptr[:-1][rows]
        offsets = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        idx = np.concatenate([self.idx[ptr[r]:ptr[r + 1]] for r in rows]) if len(rows) else np.zeros(0, np.int64)
        return np.asarray(self.users, np.int64)[rows], offsets, idx


class PPO:
    """The PPO loop.  `policy` offers act(obs, deterministic, row) -> (words [1, W], value, logp), value_of(obs) and
    evaluate(users, offsets, idx, words) -> (values, logp, ent) [B], plus .dtype / .device; `env` offers reset() -> obs and
    step(action [I] of 0/1, numpy) -> (obs, reward, done).  ent_decay_every / ent_decay: the reference's EntropyScheduler
    (ent_coef *= decay whenever num_timesteps % every == 0); log_reward_stats: the reference's RewardNormalizer as SB3 runs it -- called after
    the returns exist, so it records the rollout's reward statistics and changes nothing PPO reads."""

    def __init__(self, policy, env, learning_rate=3e-4, n_steps=2048, batch_size=64, n_epochs=10, gamma=0.99, gae_lambda=0.95, clip_range=0.2,
                 ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5, target_kl=None, ent_decay_every=None, ent_decay=0.9, log_reward_stats=False):
        self.policy, self.env = policy, env
        self.n_steps, self.batch_size, self.n_epochs = int(n_steps), int(batch_size), int(n_epochs)
        self.gamma, self.gae_lambda, self.clip_range = gamma, gae_lambda, clip_range
        self.ent_coef, self.vf_coef, self.max_grad_norm, self.target_kl = ent_coef, vf_coef, max_grad_norm, target_kl
        self.ent_decay_every, self.ent_decay, self.log_reward_stats = ent_decay_every, ent_decay, log_reward_stats
        self.optimizer = torch.optim.Adam(policy.parameters(), lr=learning_rate, eps=1e-5)
        self.buffer = RolloutBuffer(self.n_steps)
        self.num_timesteps, self.n_rollouts = 0, 0
        self.reward_stats, self.update_log = [], []
        self._last_obs, self._last_start = None, 1.0

    def collect_rollout(self):
        if self._last_obs is None:
            self._last_obs, self._last_start = self.env.reset(), 1.0
        buf = self.buffer
        buf.reset()
        done = False
        for t in range(self.n_steps):
            with torch.no_grad():
                words, value, logp = self.policy.act(self._last_obs, deterministic=False, row=t, call=self.n_rollouts)
            action = policyhead.unpack_bits(words, self.policy.item_num)[0].cpu().numpy().astype(np.int64)
            kept = (self._last_obs[0], np.array(self._last_obs[1], np.int64))
            obs, reward, done = self.env.step(action)
            self.num_timesteps += 1
            if self.ent_decay_every and self.num_timesteps % self.ent_decay_every == 0:
                self.ent_coef *= self.ent_decay
            buf.add(kept, words, reward, self._last_start, value, logp)       # the policy's own action, not the environment's clipped profile
            if done:
                obs = self.env.reset()
            self._last_obs, self._last_start = obs, float(done)
        with torch.no_grad():
            last_value = float(self.policy.value_of(self._last_obs))
        buf.finish(last_value, float(done), self.gamma, self.gae_lambda)
        if self.log_reward_stats:
            r = np.array(buf.rewards)
            mean, std = r.mean(), r.std() + 1e-8
            self.reward_stats.append((float(mean), float(std), float(((r - mean) / std).min()), float(((r - mean) / std).max())))
        self.n_rollouts += 1

    def train(self):
        buf, pol = self.buffer, self.policy
        n = len(buf.rewards)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=pol.dtype, device=pol.device)
        adv_all, ret_all, old_all = t(buf.advantages), t(buf.returns), t(buf.logps)
        log = dict(epochs=0, steps=0, stopped=False, kl=[], loss=[])
        for epoch in range(self.n_epochs):
            order = np.random.permutation(n)
            for lo in range(0, n, self.batch_size):
                rows = order[lo:lo + self.batch_size]
                users, offsets, idx = buf.observations(rows)
                sel = torch.as_tensor(rows, device=buf.actions.device)
                values, logp, ent = pol.evaluate(users, offsets, idx, buf.actions[sel].contiguous())
                sel = sel.to(pol.device)
                loss, kl = ppo_minibatch_loss(logp, old_all[sel], ent, values, adv_all[sel], ret_all[sel], self.clip_range, self.ent_coef, self.vf_coef)
                log['kl'].append(kl); log['loss'].append(float(loss.detach()))
                if self.target_kl is not None and kl > 1.5 * self.target_kl:
                    log['stopped'] = True
                    break
                self.optimizer.zero_grad()
                loss.backward()
                nn.utils.clip_grad_norm_(pol.parameters(), self.max_grad_norm)
                self.optimizer.step()
                log['steps'] += 1
            if log['stopped']:
                break
            log['epochs'] += 1
        self.update_log.append(log)
        return log

    def learn(self, total_timesteps):
        while self.num_timesteps < total_timesteps:
            self.collect_rollout()
            self.train()
        return self


# ------------------------------------------------------------------------------------------------ policies
def _orthogonal(module, gain):
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.orthogonal_(m.weight, gain=gain)
            nn.init.zeros_(m.bias)


def _tower(n_in, width=64):
    return nn.Sequential(nn.Linear(n_in, width), nn.Tanh(), nn.Linear(width, width), nn.Tanh())


class _PolicyBase(nn.Module):
    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    def _t(self, a, dtype=torch.long):
        return torch.as_tensor(np.asarray(a), dtype=dtype, device=self.device)


class PoisonRecPolicy(_PolicyBase):
    """The repaired CustomPolicy (PoisonRec.py:197-401).  Query: E_u = user_embedding[userId], E_i = the MEAN of the item table's rows over the
    profile's items, the length-2 sequence (E_u, E_i) -- one per observation -- through LSTM(dim, dim, 2), q = DNN(h_last); the head is
    Bernoulli(logits = softmax(q E^T)) over the item table E (policyhead).  Value: SB3's combined extractor (one-hot userId, multi-hot itemInteract)
    into Linear(F + I, 64) - tanh - Linear(64, 64) - tanh - Linear(64, 1), the first layer formed sparsely as
    W_user[userId] + sum_(i in profile) W_item[i] + b.  Init as _build gives it: orthogonal with gain sqrt 2 (value tower), 0.01 (the DNN), 1 (the value
    head), biases 0; the LSTM and the two embeddings keep torch's defaults."""

    def __init__(self, fake_num, item_num, dim=64, route='composed', noise_source='torch', seed=0):
        super().__init__()
        self.fake_num, self.item_num, self.dim = int(fake_num), int(item_num), int(dim)
        self.route, self.noise_source, self.seed = route, noise_source, int(seed)
        self.user_embedding = nn.Embedding(self.fake_num, self.dim)
        self.item_embedding = nn.Embedding(self.item_num, self.dim)
        self.LSTM = nn.LSTM(input_size=self.dim, hidden_size=self.dim, num_layers=2)
        self.DNN = nn.Sequential(nn.Linear(self.dim, self.dim), nn.ReLU(), nn.Linear(self.dim, self.dim))
        first = nn.Linear(self.fake_num + self.item_num, 64)
        nn.init.orthogonal_(first.weight, gain=2 ** 0.5)
        self.vf_user = nn.Parameter(first.weight.detach()[:, :self.fake_num].t().contiguous())
        self.vf_item = nn.Parameter(first.weight.detach()[:, self.fake_num:].t().contiguous())
        self.vf_bias = nn.Parameter(torch.zeros(64))
        self.vf_second = nn.Linear(64, 64)
        self.value_net = nn.Linear(64, 1)
        _orthogonal(self.vf_second, 2 ** 0.5)
        _orthogonal(self.DNN, 0.01)
        _orthogonal(self.value_net, 1.0)

    def item_bag(self, offsets, idx):
        """[B, dim]: the mean of the item table's rows over each profile (an empty profile gives 0)."""
        return Fn.embedding_bag(idx, self.item_embedding.weight, offsets, mode='mean')

    def query(self, users, offsets, idx):
        seq = torch.stack([self.user_embedding(users), self.item_bag(offsets, idx)], 0)          # [2, B, dim]: every row its own sequence
        h, _ = self.LSTM(seq)
        return self.DNN(h[-1])

    def value_first_layer(self, users, offsets, idx):
        return self.vf_user[users] + Fn.embedding_bag(idx, self.vf_item, offsets, mode='sum') + self.vf_bias

    def values(self, users, offsets, idx):
        return self.value_net(torch.tanh(self.vf_second(torch.tanh(self.value_first_layer(users, offsets, idx)))))[:, 0]

    def _obs(self, obs):
        return self._t([obs[0]]), self._t([0]), self._t(obs[1])

    def value_of(self, obs):
        return self.values(*self._obs(obs))[0]

    def act(self, obs, deterministic=False, row=0, call=0):
        users, offsets, idx = self._obs(obs)
        q, E = self.query(users, offsets, idx).contiguous(), self.item_embedding.weight.detach()
        fused = self.route == 'fused'
        sample = policyhead.bernoulli_softmax_sample if fused else policyhead.bernoulli_softmax_sample_composed
        if deterministic:
            words, logp, _ = sample(q, E, deterministic=True)
        elif self.noise_source == 'hash':
            words, logp, _ = sample(q, E, seed=self.seed, call=call, row0=row)
        else:
            words, logp, _ = sample(q, E, u=torch.rand(1, self.item_num, dtype=self.dtype, device=self.device))
        return words, self.values(users, offsets, idx)[0], logp[0]

    def evaluate(self, users, offsets, idx, words):
        users, offsets, idx = self._t(users), self._t(offsets), self._t(idx)
        q = self.query(users, offsets, idx)
        logp, ent = policyhead.bernoulli_softmax_head(q, self.item_embedding.weight, words.to(self.device), route=self.route)
        return self.values(users, offsets, idx), logp, ent


class MlpBernoulliPolicy(_PolicyBase):
    """SB3's 'MlpPolicy' on a MultiBinary observation and action (RLAttack): separate pi and vf towers Linear(I, 64) - tanh - Linear(64, 64) - tanh,
    the action head Linear(64, I) gives the Bernoulli logits, the value head is Linear(64, 1); orthogonal init with gains sqrt 2, 0.01 and 1."""

    def __init__(self, item_num):
        super().__init__()
        self.item_num = int(item_num)
        self.pi, self.vf = _tower(self.item_num), _tower(self.item_num)
        self.action_net, self.value_net = nn.Linear(64, self.item_num), nn.Linear(64, 1)
        _orthogonal(self.pi, 2 ** 0.5); _orthogonal(self.vf, 2 ** 0.5); _orthogonal(self.action_net, 0.01); _orthogonal(self.value_net, 1.0)

    def _dense(self, offsets, idx, B):
        x = torch.zeros(B, self.item_num, dtype=self.dtype, device=self.device)
        lens = torch.diff(torch.cat([offsets, offsets.new_tensor([idx.numel()])]))
        x[torch.repeat_interleave(torch.arange(B, device=self.device), lens), idx] = 1
        return x

    def _heads(self, x):
        return self.action_net(self.pi(x)), self.value_net(self.vf(x))[:, 0]

    def value_of(self, obs):
        return self._heads(self._dense(self._t([0]), self._t(obs[1]), 1))[1][0]

    def act(self, obs, deterministic=False, row=0, call=0):
        logits, value = self._heads(self._dense(self._t([0]), self._t(obs[1]), 1))
        probs = torch.sigmoid(logits)
        a = torch.round(probs) if deterministic else torch.bernoulli(probs)
        logp = -Fn.binary_cross_entropy_with_logits(logits, a, reduction='none').sum(1)
        return policyhead.pack_bits(a), value[0], logp[0]

    def evaluate(self, users, offsets, idx, words):
        offsets, idx = self._t(offsets), self._t(idx)
        logits, values = self._heads(self._dense(offsets, idx, len(users)))
        a = policyhead.unpack_bits(words.to(self.device), self.item_num).to(self.dtype)
        logp = -Fn.binary_cross_entropy_with_logits(logits, a, reduction='none').sum(1)
        ent = Fn.binary_cross_entropy_with_logits(logits, torch.sigmoid(logits), reduction='none').sum(1)
        return values, logp, ent


# ------------------------------------------------------------------------------------------------ environments
def inject_fake_users(recommender, fake_num, targets):
    """fakeUserInject of both attacks (PoisonRec.py:87-122): the fake users join the data with the target items as their only interactions, the
    recommender is re-created on the extended data and keeps its trained tables in the leading rows."""
    Pu, Pi = recommender.model()
    data = recommender.data
    first = data.user_num
    data.user_num += fake_num
    for i in range(fake_num):
        data.user['fakeuser{}'.format(i)] = len(data.user)
        data.id2user[len(data.user) - 1] = 'fakeuser{}'.format(i)
    for u in range(first, first + fake_num):
        append_rows(data, [(data.id2user[u], data.id2item[i]) for i in targets])
    _, _, data.interaction_mat = rebuild_interaction_matrix(data)
    recommender.__init__(recommender.args, data)
    with torch.no_grad():
        emb = recommender.model.embedding_dict
        emb['user_emb'][:Pu.shape[0]] = Pu.detach().to(emb['user_emb'].device)
        emb['item_emb'][:] = Pi.detach().to(emb['item_emb'].device)
    if torch.cuda.is_available():
        recommender.model = recommender.model.cuda()
    recommender.user_emb, recommender.item_emb = recommender.model.embedding_dict['user_emb'], recommender.model.embedding_dict['item_emb']


class ShillingEnv:
    """MyEnv of both attacks.  One episode is F steps, step t acts for fake user t.  The observation is (userId, the item ids of the previous step's
    final profile), initially (0, the targets).  step(action): when more than n_keep bits are set, np.random.choice(ones, size=n_keep, replace=False)
    on the global numpy generator keeps n_keep of them; the targets are added; the graph becomes the data's matrix with fake user t's row replaced
    by the profile (the other fake users keep their injected rows, as the reference's copy-then-assign does).  every_step=False (PoisonRec): the
    reward is 0 until the last step, where the recommender is retrained for retrain_epochs with Adam(lr = lRate / 10) and the reward is
    hitRate@50 * user_num; the graph is rebuilt at that step only, since nothing reads it before.  every_step=True (RLAttack): every step rebuilds,
    retrains and is rewarded."""

    def __init__(self, item_num, fakeUser, maliciousFeedbackNum, recommender, targetItem, every_step=False, retrain_epochs=10):
        self.item_num, self.fakeUser, self.fakeUserNum = int(item_num), list(fakeUser), len(fakeUser)
        self.maliciousFeedbackNum, self.recommender, self.targetItem = int(maliciousFeedbackNum), recommender, list(targetItem)
        self.every_step, self.retrain_epochs = every_step, int(retrain_epochs)
        self.itemList = np.array(sorted(set(self.targetItem)), np.int64)
        self.fakeUserDone, self.fakeUserid = False, 0
        self.retrain_seconds = 0.0
        self._real = None

    def reset(self):
        self.itemList = np.array(sorted(set(self.targetItem)), np.int64)
        if self.fakeUserDone:
            self.fakeUserDone, self.fakeUserid = False, 0
        return 0, self.itemList.copy()

    def profile(self, action):
        """The step's final item list from the policy's action: the literal numpy calls of the reference's step."""
        action = np.asarray(action)
        ones_indices = np.where(action == 1)[0]
        if len(ones_indices) > self.maliciousFeedbackNum:
            keep_indices = np.random.choice(ones_indices, size=self.maliciousFeedbackNum, replace=False)
            action = np.zeros_like(action)
            action[keep_indices] = 1
        state = np.zeros(self.item_num)
        state[np.where(action == 1)[0]] = 1
        state[self.targetItem] = 1
        return np.where(state == 1)[0]

    def set_fake_row(self, fake_id, items):
        rec = self.recommender
        U = self.fakeUser[0]
        if self._real is None:
            base = sp.csr_matrix(rec.data.matrix(), dtype=np.float32)
            self._real, self._fake = base[:U], base[U:].tolil()
        block = self._fake.copy()
        block.rows[fake_id], block.data[fake_id] = [int(i) for i in items], [1.0] * len(items)
        ui = sp.vstack([self._real, block.tocsr()], format='csr', dtype=np.float32)
        init_graph(rec.model, ui, U + self.fakeUserNum, self.item_num, n_real=U)

    def reward(self):
        import time
        rec = self.recommender
        t0 = time.perf_counter()
        optimizer = torch.optim.Adam(rec.model.parameters(), lr=rec.args.lRate / 10)
        with contextlib.redirect_stdout(io.StringIO()):
            rec.train(Epoch=self.retrain_epochs, optimizer=optimizer, evalNum=1)
        r = AttackMetric(rec, self.targetItem, [50]).hitRate()[0] * rec.data.user_num
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.retrain_seconds += time.perf_counter() - t0
        return r

    def step(self, action):
        self.itemList = self.profile(action)
        last = self.fakeUserid == self.fakeUserNum - 1
        if self.every_step or last:
            self.set_fake_row(self.fakeUserid, self.itemList)
        if last:
            self.fakeUserDone = True
        reward = self.reward() if (self.every_step or self.fakeUserDone) else 0
        self.fakeUserid = (self.fakeUserid + 1) % self.fakeUserNum
        user = 0 if self.every_step else self.fakeUserid
        return (user, self.itemList.copy()), reward, self.fakeUserDone


def run_final_episode(policy, env, real_rows, fake_num, item_num):
    """The attacks' closing deterministic episode (PoisonRec.py:73-85): each step's profile is written to the row of the environment's fakeUserid
    AFTER the step, i.e. of fake user (t + 1) % F, as the reference does.  Returns the (U + F) x I matrix."""
    obs, done = env.reset(), False
    rows = [np.zeros(0, np.int64)] * fake_num
    t = 0
    while not done:
        with torch.no_grad():
            words, _, _ = policy.act(obs, deterministic=True, row=t)
        obs, _, done = env.step(policyhead.unpack_bits(words, item_num)[0].cpu().numpy().astype(np.int64))
        rows[env.fakeUserid] = env.itemList.copy()
        t += 1
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    block = sp.csr_matrix((np.ones(ptr[-1], np.float32), np.concatenate(rows), ptr), shape=(fake_num, item_num), dtype=np.float32)
    return sp.vstack([sp.csr_matrix(real_rows, dtype=np.float32), block], format='csr', dtype=np.float32)


def hash_seed():
    """One seed per attack for the counter-hash noise, from Python's random (as GSPAttack draws its own)."""
    return random.getrandbits(63)

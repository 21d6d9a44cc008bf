"""PoisonRec -- the attack the reference's attack/Black/PoisonRec.py describes, with PPO written out (attack/Black/_ppo.py: no gym, no
stable_baselines3) and the policy head on the MI355X kernel.  A PPO agent builds the fake profiles one fake user per step; the reward of an episode
is hitRate@50 * user_num of the target items after the victim recommender has been retrained on the poisoned graph.  Same constructor attributes and
protocol: `posionDataAttack(recommender)` returns the (U + F) x I scipy matrix, also stored in `self.interact`.

PPO settings (PoisonRec.py:67-72): lr 0.01, clip 0.1, target_kl 0.03, ent_coef 0.1 multiplied by 0.9 whenever num_timesteps % 100 == 0, gamma 1,
n_steps = batch_size = F, 5 epochs, vf_coef 0.5, max_grad_norm 0.5, F * 100 timesteps (attribute total_timesteps).

The reference's file has defects as written; these three repairs give the attack it describes:
  1. One distribution for the whole training batch (PoisonRec.py:203-209): in the rollout (one observation) the extractor builds a length-2 sequence
     (E_u, E_i); in evaluate_actions (B observations, userId [B, 1]) vstack builds ONE sequence of length 2B with batch 1, the head returns a single
     row and broadcasts it against all B actions, so the new log-probabilities are not those of the policy that acted and the PPO ratio means nothing.
     Here every row is its own length-2 sequence, exactly as the rollout computed it.
  2. Bag of 0/1 indices (PoisonRec.py:205): EmbeddingBag receives the multi-hot vector itself as indices and averages rows 0 and 1 of the table,
     weighted by the profile's size.  Here the bag is the mean of the table rows of the interacted items.
  3. Undefined attribute (PoisonRec.py:49): self.item_num is read before it exists.  Here a fractional maliciousFeedbackSize uses data.item_num.

Kept as the reference computes them:
  * Bernoulli(logits = softmax(.)) (PoisonRec.py:363-364, 400): the logits are probabilities, so every item's pick probability lies in
    [0.5, 0.731]; the deterministic mode round(sigmoid(p)) picks every item whose p has not underflowed to 0, and the environment's random cut
    (np.random.choice on the global numpy generator) decides most of a profile.  It runs, and it is what the file's code says.
  * RewardNormalizer (PoisonRec.py:403-420): SB3 calls on_rollout_end after the returns and advantages exist, so the callback changes nothing
    PPO reads (applied earlier it would map every rollout's [0, ..., 0, r] to the same vector whatever r is).  Here it records the statistics
    (agent.reward_stats) and leaves the buffer alone.
  * The environment's graph at a step is the injected data with ONE fake row replaced (uiAdj[:, :] is a copy), and the closing episode writes step
    t's profile to fake user (t + 1) % F (env.fakeUserid has advanced when it is read).

Mechanics: the head softmax(DNN(h) E^T) over every (fake user, item) pair, its Bernoulli log-probability and entropy and their gradients stream
through ops.bernoulli_softmax_head / ops.bernoulli_softmax_sample (csrc/arl_policyhead.hip) -- no F x I tensor exists.  policy_route 'fused' (the
default on a GPU where the kernel takes the shape) runs the kernels, 'composed' (the default elsewhere, the only route on the CPU) the torch panels.
noise_source 'torch' (the default) draws torch.rand(1, I) per step; 'hash' draws one seed per attack from Python's random and takes the uniforms
from a counter hash of (seed, rollout, step, item) inside the kernel.  The LSTM, the DNN and the value net are plain torch; the value net's first
layer is formed sparsely (W_user[userId] + sum of W_item rows + b), observations are index lists and actions packed bits.  Single GPU, fp32."""
import numpy as np
import scipy.sparse as sp
import torch

from ... import policyhead
from .._common import AttackBase
from . import _ppo


class PoisonRec(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = True

    def __init__(self, arg, data, dim=64):
        super().__init__(arg, data)
        self.maliciousFeedbackNum = int(self.maliciousFeedbackNum)
        self.env = None
        self.item_num = data.item_num
        self.fakeUser = list(range(self.userNum, self.userNum + self.fakeUserNum))
        self.isNormalized = True
        self.dim = int(dim)
        self.total_timesteps = self.fakeUserNum * 100
        self.retrain_epochs = 10                         # Epoch of the environment's recommender.train
        self.seed = None                                 # an int seeds torch, numpy and Python's random at the start of posionDataAttack
        self.noise_source = 'torch'
        on_gpu = torch.cuda.is_available() and policyhead.bernoulli_softmax_supported(max(self.fakeUserNum, 1), self.item_num, self.dim)
        self.policy_route = 'fused' if on_gpu else 'composed'
        self.agent = None

    def _build(self, recommender):
        if self.policy_route not in ('fused', 'composed'):
            raise ValueError("PoisonRec: policy_route is 'fused' or 'composed', not %r" % (self.policy_route,))
        if self.noise_source not in ('torch', 'hash'):
            raise ValueError("PoisonRec: noise_source is 'torch' or 'hash', not %r" % (self.noise_source,))
        if self.fakeUserNum < 1:
            raise ValueError('PoisonRec: at least one fake user needed')
        device = 'cuda' if torch.cuda.is_available() else 'cpu'
        if self.policy_route == 'fused' and device != 'cuda':
            raise RuntimeError("PoisonRec: policy_route 'fused' needs the GPU")
        if self.noise_source == 'hash' and device != 'cuda':
            raise RuntimeError("PoisonRec: noise_source 'hash' needs the GPU")
        policy = _ppo.PoisonRecPolicy(self.fakeUserNum, self.item_num, self.dim, route=self.policy_route, noise_source=self.noise_source,
                                      seed=_ppo.hash_seed() if self.noise_source == 'hash' else 0).to(device)
        self.env = self._env(recommender)
        self.agent = _ppo.PPO(policy, self.env, learning_rate=0.01, n_steps=self.fakeUserNum, batch_size=self.fakeUserNum, n_epochs=5, gamma=1,
                              clip_range=0.1, target_kl=0.03, ent_coef=0.1, vf_coef=0.5, max_grad_norm=0.5, ent_decay_every=100, ent_decay=0.9,
                              log_reward_stats=self.isNormalized)

    def _env(self, recommender):
        return _ppo.ShillingEnv(self.item_num, self.fakeUser, self.maliciousFeedbackNum, recommender, self.targetItem, every_step=False,
                                retrain_epochs=self.retrain_epochs)

    def posionDataAttack(self, recommender):
        if self.seed is not None:
            from ...util.tool import seedSet
            seedSet(int(self.seed))
        self.recommender = recommender
        real = sp.csr_matrix(self.interact, dtype=np.float32)[:self.userNum]
        self.fakeUserInject(recommender)
        if self.env is None:
            self._build(recommender)
            self.agent.learn(total_timesteps=self.total_timesteps)
        self.env = self._env(recommender)
        self.interact = _ppo.run_final_episode(self.agent.policy, self.env, real, self.fakeUserNum, self.item_num)
        return self.interact

    def fakeUserInject(self, recommender):
        _ppo.inject_fake_users(recommender, self.fakeUserNum, self.targetItem)
        self.fakeUser = list(range(self.userNum, self.userNum + self.fakeUserNum))

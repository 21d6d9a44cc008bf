"""RLAttack -- mirror of the reference's attack/Black/RLAttack.py with PPO written out (attack/Black/_ppo.py: no gym, no stable_baselines3).
A PPO agent with SB3's 'MlpPolicy' picks one fake user's profile per step from the multi-hot profile of the previous step; EVERY step rebuilds the
graph, retrains the victim recommender for 10 epochs and is rewarded with hitRate@50 * user_num (RLAttack.py:156-174); the episode ends after the last
fake user.  Same constructor attributes and protocol: `posionDataAttack(recommender)` returns the (U + F) x I scipy matrix, also stored in
`self.interact`.

PPO settings (RLAttack.py:59-60): 'MlpPolicy', clip 0.1, gamma 1, n_steps 20, 10 epochs, and SB3's defaults for the rest (lr 3e-4, batch_size 64,
gae_lambda 0.95, ent_coef 0, vf_coef 0.5, max_grad_norm 0.5, no target_kl); 400 timesteps (attribute total_timesteps).

Repair: self.item_num is read before it exists (RLAttack.py:44); a fractional maliciousFeedbackSize uses data.item_num.
Kept: the environment's graph at a step is the injected data with one fake row replaced, and the closing episode writes step t's profile to fake
user (t + 1) % F, as in PoisonRec.

The policy is three small Linear layers on at most 64 rows: it stays plain torch and has no kernel.  The retraining and the scoring run on the
engine and ops.score_mask_topk like every other attack's."""
import numpy as np
import scipy.sparse as sp
import torch

from .._common import AttackBase
from . import _ppo


class RLAttack(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = True

    def __init__(self, arg, data):
        super().__init__(arg, data)
        self.maliciousFeedbackNum = int(self.maliciousFeedbackNum)
        self.env = None
        self.item_num = data.item_num
        self.fakeUser = list(range(self.userNum, self.userNum + self.fakeUserNum))
        self.total_timesteps = 400
        self.retrain_epochs = 10                         # Epoch of the environment's recommender.train
        self.seed = None                                 # an int seeds torch, numpy and Python's random at the start of posionDataAttack
        self.agent = None

    def _env(self, recommender):
        return _ppo.ShillingEnv(self.item_num, self.fakeUser, self.maliciousFeedbackNum, recommender, self.targetItem, every_step=True,
                                retrain_epochs=self.retrain_epochs)

    def posionDataAttack(self, recommender):
        if self.fakeUserNum < 1:
            raise ValueError('RLAttack: at least one fake user needed')
        if self.seed is not None:
            from ...util.tool import seedSet
            seedSet(int(self.seed))
        self.recommender = recommender
        real = sp.csr_matrix(self.interact, dtype=np.float32)[:self.userNum]
        self.fakeUserInject(recommender)
        if self.env is None:
            self.env = self._env(recommender)
            policy = _ppo.MlpBernoulliPolicy(self.item_num).to('cuda' if torch.cuda.is_available() else 'cpu')
            self.agent = _ppo.PPO(policy, self.env, clip_range=0.1, gamma=1, n_steps=20, n_epochs=10)
            self.agent.learn(total_timesteps=self.total_timesteps)
        self.env = self._env(recommender)
        self.interact = _ppo.run_final_episode(self.agent.policy, self.env, real, self.fakeUserNum, self.item_num)
        return self.interact

    def fakeUserInject(self, recommender):
        _ppo.inject_fake_users(recommender, self.fakeUserNum, self.targetItem)
        self.fakeUser = list(range(self.userNum, self.userNum + self.fakeUserNum))

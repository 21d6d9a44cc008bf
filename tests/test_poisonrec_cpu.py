"""PoisonRec and RLAttack without a GPU: the composed head and the bit packing against the restatement (tests/poisonrec_restatement.py), the three
repairs (per-row sequences, the item bag's mean, data.item_num), the sparse value tower, the environment's step against the literal numpy calls,
both attacks end to end on a synthetic data set with a stub recommender, and the C entries' exports and argument checks."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn as nn
from conftest import ROOT
from test_shilling_cpu import attack_args
import poisonrec_restatement as rs


# ------------------------------------------------------------------------------------------------ the head and the packing
@pytest.mark.parametrize('I', [1, 31, 32, 33, 77])
def test_pack_bits_round_trip_and_pad_bits(I):
    from arlib_amd import policyhead as ph
    a = torch.rand(5, I, generator=torch.Generator().manual_seed(I)) < 0.5
    a[0], a[-1] = True, False
    w = ph.pack_bits(a)
    assert w.dtype == torch.int32 and w.shape == (5, (I + 31) // 32) and torch.equal(w, rs.pack(a.numpy()))
    assert torch.equal(ph.unpack_bits(w, I), a) and torch.equal(ph.pack_bits(a.float() * 3), w)
    if I % 32:
        assert int(((w[:, -1].long() & 0xFFFFFFFF) >> (I % 32)).abs().max()) == 0           # pad bits are zero, also in the all-ones row
    with pytest.raises(ValueError):
        ph.unpack_bits(w, I + 32)


@pytest.mark.parametrize('B,I,d', [(1, 1, 16), (3, 77, 16), (9, 130, 48)])
def test_composed_head_against_the_restatement(B, I, d):
    from arlib_amd import policyhead as ph
    g = torch.Generator().manual_seed(B + I)
    q, E = torch.randn(B, d, generator=g), torch.randn(I, d, generator=g) / d ** 0.5
    a = torch.rand(B, I, generator=g) < 0.5
    gl, ge, u = torch.randn(B, generator=g), torch.randn(B, generator=g), torch.rand(B, I, generator=g)
    want = rs.head(q, E, a, gl, ge)
    words = ph.pack_bits(a)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, 2e-6)):
        got = ph.bernoulli_softmax_eval_composed(q.to(dtype), E.to(dtype), words, gl.to(dtype), ge.to(dtype), want_grad=True, chunk=2)
        for x, w in zip(got, want):
            assert float((x.double() - w).abs().max()) <= tol * max(float(w.abs().max()), 1e-30)
        ql, El = q.to(dtype).requires_grad_(), E.to(dtype).requires_grad_()
        logp, ent = ph.bernoulli_softmax_head(ql, El, words)                                # 'auto' on the CPU: the composed route, through autograd
        (gl.to(dtype) * logp + ge.to(dtype) * ent).sum().backward()
        assert float((ql.grad.double() - want[2]).abs().max()) <= tol * float(want[2].abs().max() + 1e-30)
        assert float((El.grad.double() - want[3]).abs().max()) <= tol * float(want[3].abs().max() + 1e-30)
    a64, logp64, count64, gap, _ = rs.sample(q, E, u)
    assert gap > 1e-6
    sw, sl, sc = ph.bernoulli_softmax_sample_composed(q, E, u=u, chunk=2)
    assert torch.equal(sw, rs.pack(a64.numpy())) and torch.equal(sc.long(), count64) and float((sl.double() - logp64).abs().max()) <= 1e-5 * I
    dw, _, dc = ph.bernoulli_softmax_sample_composed(q, E, deterministic=True)
    assert dc.tolist() == [I] * B                                                            # every p is positive here: every item is picked
    with pytest.raises(ValueError):
        ph.bernoulli_softmax_sample_composed(q, E)
    from arlib_amd import _lib
    with pytest.raises(_lib.ArlError):
        ph.bernoulli_softmax_head(q, E, words, route='fused')                                # the kernels take device tensors only


# ------------------------------------------------------------------------------------------------ the policy
def small_policy(F=4, I=37, dim=16, seed=1):
    from arlib_amd.attack.Black import _ppo
    torch.manual_seed(seed)
    return _ppo.PoisonRecPolicy(F, I, dim).double()


def observations(F, I, seed=2):
    rng = np.random.default_rng(seed)
    profiles = [np.sort(rng.choice(I, size=int(rng.integers(1, 9)), replace=False)) for _ in range(F + 2)]
    users = np.array([b % F for b in range(F + 2)], np.int64)
    offsets = np.concatenate([[0], np.cumsum([len(p) for p in profiles])[:-1]]).astype(np.int64)
    return users, offsets, np.concatenate(profiles), profiles


def test_repaired_policy_rows_are_their_own_sequences():
    """Repair 1: row b of a B-row evaluation equals the single-row rollout evaluation of the same observation, and both equal the restatement."""
    pol = small_policy()
    users, offsets, idx, profiles = observations(4, 37)
    T = lambda a: torch.as_tensor(a)
    with torch.no_grad():
        q = pol.query(T(users), T(offsets), T(idx))
        v = pol.values(T(users), T(offsets), T(idx))
        for b in range(len(users)):
            q1 = pol.query(T(users[b:b + 1]), T([0]), T(profiles[b]))
            assert float((q[b] - q1[0]).abs().max()) <= 1e-12
            want = rs.policy_query(pol.user_embedding.weight, pol.item_embedding.weight, pol.LSTM, pol.DNN[0], pol.DNN[2], int(users[b]), profiles[b])
            assert float((q[b] - want).abs().max()) <= 1e-12
            assert abs(float(pol.value_of((int(users[b]), profiles[b])) - v[b])) <= 1e-12
    # and through evaluate(): the log-probability of row b does not depend on the other rows of the batch
    from arlib_amd import policyhead as ph
    words = ph.pack_bits(torch.rand(len(users), 37, generator=torch.Generator().manual_seed(3)) < 0.5)
    with torch.no_grad():
        _, logp, ent = pol.evaluate(users, offsets, idx, words)
        _, logp1, ent1 = pol.evaluate(users[2:3], np.array([0]), profiles[2], words[2:3])
    assert abs(float(logp[2] - logp1[0])) <= 1e-12 and abs(float(ent[2] - ent1[0])) <= 1e-12
    assert float(logp.std()) > 0                                                             # not one broadcast row


def test_item_bag_is_the_mean_of_the_interacted_rows():
    """Repair 2."""
    pol = small_policy()
    users, offsets, idx, profiles = observations(4, 37)
    bag = pol.item_bag(torch.as_tensor(offsets), torch.as_tensor(idx))
    for b, p in enumerate(profiles):
        assert float((bag[b] - pol.item_embedding.weight[torch.as_tensor(p)].mean(0)).abs().max()) <= 1e-12


def test_sparse_value_tower_equals_the_dense_linear():
    pol = small_policy()
    F, I = 4, 37
    users, offsets, idx, profiles = observations(F, I)
    x = torch.zeros(len(users), F + I, dtype=torch.float64)
    for b, p in enumerate(profiles):
        x[b, users[b]] = 1                                                                   # the one-hot userId ...
        x[b, F + torch.as_tensor(p)] = 1                                                     # ... concatenated with the multi-hot itemInteract
    W = torch.cat([pol.vf_user, pol.vf_item], 0).t()                                        # the Linear(F + I, 64) weight
    dense = x @ W.t() + pol.vf_bias
    sparse = pol.value_first_layer(torch.as_tensor(users), torch.as_tensor(offsets), torch.as_tensor(idx))
    assert float((dense - sparse).abs().max()) <= 1e-12
    # the init _build gives: orthogonal rows of gain sqrt 2 for the tower's first layer, biases 0
    G = W @ W.t() if W.shape[0] <= W.shape[1] else W.t() @ W
    assert float((G - 2 * torch.eye(G.shape[0], dtype=torch.float64)).abs().max()) <= 1e-5
    assert float(pol.vf_bias.abs().max()) == 0 and float(pol.DNN[0].weight.abs().max()) < 0.02 and float(pol.DNN[0].bias.abs().max()) == 0


def test_module_docstrings_list_the_repairs():
    from arlib_amd.attack.Black import PoisonRec as m1, RLAttack as m2
    for n in range(1, 4):
        assert '\n  %d. ' % n in m1.__doc__
    for ref in ('PoisonRec.py:203-209', 'PoisonRec.py:205', 'PoisonRec.py:49', 'PoisonRec.py:363-364, 400', 'RewardNormalizer'):
        assert ref in m1.__doc__, ref
    assert 'RLAttack.py:44' in m2.__doc__ and 'no kernel' in m2.__doc__


# ------------------------------------------------------------------------------------------------ a stub recommender and the environment
class StubModel(nn.Module):
    def __init__(self, data, d=6):
        super().__init__()
        g = torch.Generator().manual_seed(17)
        self.embedding_dict = nn.ParameterDict({'user_emb': nn.Parameter(torch.randn(data.user_num, d, generator=g) * 0.1),
                                                'item_emb': nn.Parameter(torch.randn(data.item_num, d, generator=g) * 0.1)})
        self.adj, self.graph_calls = None, 0

    def forward(self):
        return self.embedding_dict['user_emb'], self.embedding_dict['item_emb']

    def _init_uiAdj(self, adj):
        self.adj, self.graph_calls = sp.csr_matrix(adj), self.graph_calls + 1


class StubRecommender:
    """train() is deterministic: every epoch pulls each table a step towards its graph neighbours."""

    def __init__(self, args, data):
        self.args, self.data, self.topN = args, data, [50]
        self.model = StubModel(data)
        self.user_emb, self.item_emb = self.model.embedding_dict['user_emb'], self.model.embedding_dict['item_emb']
        self.train_calls = getattr(self, 'train_calls', [])

    def train(self, Epoch=0, optimizer=None, evalNum=5, **kw):
        self.train_calls.append((Epoch, type(optimizer).__name__, optimizer.param_groups[0]['lr'], evalNum))
        U = self.data.user_num
        A = torch.as_tensor(self.model.adj[:U, U:].toarray(), dtype=torch.float32)
        with torch.no_grad():
            Pu, Pi = self.model.embedding_dict['user_emb'], self.model.embedding_dict['item_emb']
            for _ in range(Epoch):
                Pu += 0.002 * (A @ Pi)
                Pi += 0.002 * (A.t() @ Pu)
        self.user_emb, self.item_emb = self.model.embedding_dict['user_emb'], self.model.embedding_dict['item_emb']


def synthetic(seed=5, U=300, I=120):
    from arlib_amd.util.DataLoader import DataLoader
    rng = np.random.default_rng(seed)
    pairs = set((u, int(i)) for u in range(U) for i in rng.choice(I, 8, replace=False))
    pairs |= set((int(rng.integers(U)), i) for i in range(I))
    pairs = np.array(sorted(pairs))
    data = DataLoader.from_arrays((pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32)), dataName='poisonrec-syn', array_native=False)
    assert (data.user_num, data.item_num) == (U, I)
    return data


def build(cls_name, F=4, k=6, T=2, **kw):
    import importlib
    from arlib_amd.util.tool import seedSet
    seedSet(2018)
    data = synthetic()
    cls = getattr(importlib.import_module('arlib_amd.attack.Black.' + cls_name), cls_name)
    atk = cls(attack_args(cls_name, 'Black', maliciousUserSize=F, maliciousFeedbackSize=k, targetSize=T), data, **kw)
    rec = StubRecommender(SimpleNamespace(lRate=0.005), data)
    return atk, rec, data


def test_constructor_contract_and_item_num_repair():
    """Repair 3: a fractional maliciousFeedbackSize uses data.item_num."""
    import importlib
    from arlib_amd.util.tool import seedSet
    for name in ('PoisonRec', 'RLAttack'):
        seedSet(2018)
        data = synthetic()
        cls = getattr(importlib.import_module('arlib_amd.attack.Black.' + name), name)
        atk = cls(attack_args(name, 'Black', maliciousUserSize=0.01, maliciousFeedbackSize=0.05, targetSize=2), data)
        assert atk.maliciousFeedbackNum == int(0.05 * data.item_num) and atk.fakeUserNum == 3 and atk.item_num == data.item_num
        assert atk.fakeUser == [300, 301, 302] and atk.env is None and atk.recommenderModelRequired and not atk.recommenderGradientRequired
        assert atk.total_timesteps == (300 if name == 'PoisonRec' else 400)
    assert atk.__class__.__name__ == 'RLAttack'
    p = build('PoisonRec')[0]
    assert p.policy_route == 'composed' and p.noise_source == 'torch' and p.isNormalized and p.seed is None


@pytest.mark.parametrize('every_step', [False, True])
def test_environment_step(every_step):
    from arlib_amd.attack.Black import _ppo
    atk, rec, data = build('PoisonRec')
    _ppo.inject_fake_users(rec, 4, atk.targetItem)
    assert data.user_num == 304 and rec.model.embedding_dict['user_emb'].shape[0] == 304 and data.matrix().shape == (304, 120)
    assert (np.asarray(data.matrix()[300:].todense()).sum(1) == 2).all()                     # the fake users start with the targets only
    env = _ppo.ShillingEnv(120, atk.fakeUser, 6, rec, atk.targetItem, every_step=every_step, retrain_epochs=3)
    obs = env.reset()
    assert obs[0] == 0 and obs[1].tolist() == sorted(atk.targetItem)
    rng = np.random.default_rng(8)
    rewards = []
    for t in range(4):
        action = (rng.random(120) < (0.6 if t != 2 else 0.02)).astype(np.int64)             # step 2: fewer bits than the budget, no cut
        np.random.seed(100 + t)
        state = np.random.get_state()
        obs, reward, done = env.step(action)
        after = np.random.get_state()
        want_items, want_state = rs.env_step(action, 6, atk.targetItem, state)
        assert obs[1].tolist() == want_items.tolist() == env.itemList.tolist()
        assert all(np.array_equal(x, y) for x, y in zip(after, want_state))                  # numpy.random consumed like the literal call
        assert set(atk.targetItem) <= set(obs[1].tolist()) and len(obs[1]) <= 6 + len(atk.targetItem)
        assert (len(obs[1]) >= 6) == (t != 2) and obs[0] == (0 if every_step else (t + 1) % 4) and done == (t == 3)
        rewards.append(reward)
        if every_step or t == 3:                                                             # the graph: the data's matrix with fake row t replaced
            block = rec.model.adj[:304, 304:]
            assert sorted(block[300 + t].indices.tolist()) == obs[1].tolist()
            assert all(sorted(block[300 + o].indices.tolist()) == sorted(atk.targetItem) for o in range(4) if o != t)
            assert (block[:300] != sp.csr_matrix(atk.interact)).nnz == 0
    if every_step:
        assert all(r > 0 for r in rewards) and len(rec.train_calls) == 4 and rec.model.graph_calls == 4
    else:
        assert rewards[:3] == [0, 0, 0] and rewards[3] > 0 and len(rec.train_calls) == 1 and rec.model.graph_calls == 1
    assert rec.train_calls[-1] == (3, 'Adam', 0.005 / 10, 1)
    assert env.reset()[0] == 0 and env.fakeUserid == 0 and not env.fakeUserDone


# ------------------------------------------------------------------------------------------------ whole attacks
def run_attack(name, **attrs):
    atk, rec, data = build(name, **({'dim': 16} if name == 'PoisonRec' else {}))
    for k, v in attrs.items():
        setattr(atk, k, v)
    before = sp.csr_matrix(atk.interact).copy()
    res = atk.posionDataAttack(rec)
    return atk, rec, before, res


@pytest.mark.parametrize('name,steps', [('PoisonRec', 8), ('RLAttack', 8)])
def test_whole_attack_on_a_stub_recommender(name, steps):
    atk, rec, before, res = run_attack(name, seed=5, total_timesteps=steps, retrain_epochs=2)
    U, F, I, k, T = 300, 4, 120, 6, 2
    assert res.shape == (U + F, I) == atk.interact.shape and (sp.csr_matrix(res)[:U] != before).nnz == 0
    fake = np.asarray(sp.csr_matrix(res)[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0} and (fake[:, atk.targetItem] == 1).all()
    assert ((fake.sum(1) >= T) & (fake.sum(1) <= k + T)).all() and atk.fakeUser == list(range(U, U + F))
    if name == 'PoisonRec':
        # every pick probability is at least 1/2 over 120 items: the cut to k items applies at every step
        assert (fake.sum(1) >= k).all() and atk.agent.n_rollouts == 2 and atk.agent.num_timesteps == 8 and len(atk.agent.reward_stats) == 2
        assert atk.agent.buffer.actions.shape == (F, (I + 31) // 32) and len(rec.train_calls) == 3      # one per rollout and the closing episode
    else:
        assert atk.agent.num_timesteps == 20 and len(rec.train_calls) == 20 + F                          # n_steps = 20 per rollout, every step retrains
    again = run_attack(name, seed=5, total_timesteps=steps, retrain_epochs=2)[3]
    assert (sp.csr_matrix(res) != sp.csr_matrix(again)).nnz == 0                                        # two runs from one seed are identical
    other = run_attack(name, seed=6, total_timesteps=steps, retrain_epochs=2)[3]
    assert (sp.csr_matrix(res) != sp.csr_matrix(other)).nnz > 0


def test_routes_are_checked_before_training():
    if not torch.cuda.is_available():
        for attr, value in (('policy_route', 'fused'), ('noise_source', 'hash')):
            atk, rec, _ = build('PoisonRec', dim=16)
            setattr(atk, attr, value)
            with pytest.raises(RuntimeError):
                atk.posionDataAttack(rec)
    atk, rec, _ = build('PoisonRec', dim=16)
    atk.policy_route = 'nonsense'
    with pytest.raises(ValueError):
        atk.posionDataAttack(rec)


# ------------------------------------------------------------------------------------------------ the C layer
def test_header_exports_and_argument_checks():
    from arlib_amd import _lib, policyhead, ops
    names = ('arl_bernoulli_softmax_workspace_bytes', 'arl_bernoulli_softmax_eval_f32', 'arl_bernoulli_softmax_sample_f32', 'arl_bernoulli_uniforms_f32')
    hdr = open(os.path.join(ROOT, 'include', 'arlib_amd.h')).read()
    for name in names:
        assert name in _lib.EXPORTS and re.search(r'/\* attack/Black/PoisonRec\.py:363-371, 398-401 \*/\n[^\n]*\b%s\s*\(' % name, hdr), name
    assert ops.bernoulli_softmax is policyhead.bernoulli_softmax and ops.pack_bits is policyhead.pack_bits
    assert policyhead.POLICYHEAD_WIDTHS == (16, 32, 64, 128) and policyhead.POLICYHEAD_MAX_ROWS == (2 ** 31 - 1) // 128
    assert policyhead.bernoulli_softmax_supported(10_000, 100_000, 64) and policyhead.bernoulli_softmax_supported(1, 1, 16)
    assert not policyhead.bernoulli_softmax_supported(10, 10, 48) and not policyhead.bernoulli_softmax_supported(policyhead.POLICYHEAD_MAX_ROWS + 1, 10, 64)
    assert not policyhead.bernoulli_softmax_supported(0, 10, 64) and not policyhead.bernoulli_softmax_supported(10, 0, 64)
    L = _lib.lib()
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    big = policyhead.POLICYHEAD_MAX_ROWS + 1
    f = L.arl_bernoulli_softmax_eval_f32                       # arguments are checked before any launch: no device is needed to be told so
    assert f(None, 4, p, 4, 16, p, None, None, p, p, None, None, p, None) == -1
    assert f(p, 4, p, 4, 16, p, None, None, p, p, None, None, None, None) == -1
    assert f(p, 4, p, 4, 16, p, None, None, p, p, p, p, p, None) == -1                       # gradients without upstreams
    assert f(p, 4, p, 4, 20, p, None, None, p, p, None, None, p, None) == -2
    assert f(p, big, p, 4, 16, p, None, None, p, p, None, None, p, None) == -3
    assert f(p, 4, p, big, 16, p, None, None, p, p, None, None, p, None) == -3
    assert f(p, 0, p, 4, 16, p, None, None, p, p, None, None, p, None) == -4
    assert f(p + 4, 4, p, 4, 16, p, None, None, p, p, None, None, p, None) == -4
    s = L.arl_bernoulli_softmax_sample_f32
    assert s(p, 4, p, 4, 16, None, 1, 2, 0, 0, None, p, p, p, None) == -1
    assert s(p, 4, p, 4, 48, None, 1, 2, 0, 0, p, p, p, p, None) == -2
    assert s(p, 4, p, big, 16, None, 1, 2, 0, 0, p, p, p, p, None) == -3 and s(p, 4, p, 4, 16, None, 1, 2, 2 ** 31, 0, p, p, p, p, None) == -3
    assert s(p, 4, p, 4, 16, None, 1, 2, -1, 0, p, p, p, p, None) == -4 and s(p, 4, p + 4, 4, 16, None, 1, 2, 0, 0, p, p, p, p, None) == -4
    n = L.arl_bernoulli_uniforms_f32
    assert n(1, 2, 0, 4, 4, None, None) == -1 and n(1, 2, 0, 0, 4, p, None) == -4 and n(1, 2, 0, 4, 2 ** 31, p, None) == -3
    w = L.arl_bernoulli_softmax_workspace_bytes
    assert w(10, 10, 20, 1) == 0 and w(0, 10, 16, 1) == 0 and w(10, 0, 16, 0) == 0
    assert w(60, 3706, 64, 0) % 16 == 0 and 0 < w(60, 3706, 64, 0) <= w(60, 3706, 64, 1)
    # O(B + I) state: cfg2's shape (10 000 x 100 000 pairs, 4 GB as one fp32 matrix) needs under 128 MiB
    assert w(10_000, 100_000, 64, 1) < 2 ** 27 and w(1, 100_000, 64, 0) < 2 ** 14


def test_host_tensors_raise_in_the_op_module():
    from arlib_amd import policyhead, _lib
    q, E = torch.randn(4, 16), torch.randn(40, 16)
    words = policyhead.pack_bits(torch.zeros(4, 40))
    with pytest.raises(_lib.ArlError):
        policyhead.bernoulli_softmax_eval(q, E, words)
    with pytest.raises(_lib.ArlError):
        policyhead.bernoulli_softmax_sample(q, E, deterministic=True)
    with pytest.raises(_lib.ArlError):
        policyhead.bernoulli_uniforms(1, 2, 4, 40, device='cpu')

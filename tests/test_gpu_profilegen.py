"""GSPAttack's profile generator on the device (csrc/arl_profilegen.hip): the pair-MLP kernels and the relaxed Gumbel top-k kernels against float64
(tests/gsp_restatement.py) at ragged sizes, the counter-hash noise, exact upstream scaling, the dispatchers past the limits, and whole attacks on
the fused route.  The poisoned-memory runs are in test_gpu_profilegen_poison.py.

Bar for every value compared with float64 (the one test_gpu_gsp.py holds arl_bce_allpairs_f32 to): the max-norm relative error is at most
FACTOR = 4 times the composed fp32 torch route's own error on the same inputs, with FLOOR = 1e-6.  Measured figures: DESIGN.md section 3k."""
import functools
import math

import numpy as np
import pytest
import torch
from conftest import close
from test_gpu_gsp import attack_problem, run_device_attack, restated_attack
import gsp_restatement as rs

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FACTOR, FLOOR = 4.0, 1e-6


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def held(what, name, got, comp, want):
    want = want.detach().numpy()
    ek, ec = rel(got.detach().cpu().numpy().reshape(want.shape), want), rel(comp.detach().cpu().numpy().reshape(want.shape), want)
    print('%s %s: kernel %.3e composed %.3e' % (what, name, ek, ec))
    assert ek <= max(FACTOR * ec, FLOOR), (what, name, ek, ec)


# ------------------------------------------------------------------------------------------------ pair MLP
def pair_problem(F, I, H, seed):
    """A, B ~ N(0, 1): half of the pre-activations A[f, h] + B[i, h] are negative; up to 7 of them are forced to exactly 0 (B[i, h] = -A[f, h])."""
    g = torch.Generator().manual_seed(seed)
    A, B = torch.randn(F, H, generator=g), torch.randn(I, H, generator=g)
    w2, b2 = torch.randn(H, generator=g) / math.sqrt(H), torch.randn(1, generator=g)
    zeros = []
    for n in range(min(7, I)):
        f, i, h = n % F, (n * 37) % I, (n * 11) % H
        if all(z[1:] != (i, h) for z in zeros):
            B[i, h] = -A[f, h]
            zeros.append((f, i, h))
    up = torch.randn(F, I, generator=g)
    return A, B, w2, b2, up, zeros


def pair_float64(A, B, w2, b2, up):
    L = [t.double().requires_grad_() for t in (A, B, w2, b2)]
    x = torch.relu(L[0][:, None, :] + L[1][None]) @ L[2] + L[3]
    x.backward(up.double())
    return [x.detach()] + [t.grad for t in L]


PAIR_SHAPES = [(1, 1, 1), (3, 77, 8), (5, 1030, 41), (70, 515, 316), (2, 300, 1024)]
PAIR_NAMES = ('x', 'dA', 'dB', 'dw2', 'db2')


@pytest.mark.parametrize('F,I,H', PAIR_SHAPES)
def test_pair_mlp_against_float64(F, I, H):
    from arlib_amd import ops
    assert PAIR_SHAPES[-1][2] == ops.PAIR_MLP_MAX_H
    A, B, w2, b2, up, zeros = pair_problem(F, I, H, seed=F + I + H)
    assert zeros and all(float(A[f, h] + B[i, h]) == 0.0 for f, i, h in zeros)
    want = pair_float64(A, B, w2, b2, up)
    if F * I * H > 1000:
        assert 0.4 < float(((A[:, None, :] + B[None]) < 0).double().mean()) < 0.6

    def run(fn):
        L = [t.to(DEV).requires_grad_() for t in (A, B, w2, b2)]
        x = fn(*L)
        x.backward(up.to(DEV))
        return [x] + [t.grad for t in L]
    got, comp = run(ops.pair_mlp_logits), run(ops.pair_mlp_logits_composed)
    again = run(ops.pair_mlp_logits)
    for name, k, c, w, k2 in zip(PAIR_NAMES, got, comp, want, again):
        assert k.shape == c.shape and torch.equal(k, k2)                         # fixed-order sums: the same bits from run to run
        held('pair_mlp F=%d I=%d H=%d' % (F, I, H), name, k, c, w)


def test_pair_mlp_relu_derivative_at_zero_is_zero():
    from arlib_amd import ops
    A = torch.tensor([[1.0, -2.0]], device=DEV, requires_grad=True)
    B = torch.tensor([[-1.0, 2.0], [0.5, 0.5]], device=DEV, requires_grad=True)                # item 0: both pre-activations exactly 0
    w2, b2 = torch.tensor([3.0, 5.0], device=DEV), torch.zeros(1, device=DEV)
    x = ops.pair_mlp_logits(A, B, w2, b2)
    assert x.tolist() == [[0.0, 4.5]]
    x.sum().backward()
    assert A.grad.tolist() == [[3.0, 0.0]] and B.grad.tolist() == [[0.0, 0.0], [3.0, 0.0]]


# ------------------------------------------------------------------------------------------------ Gumbel top-k with a caller's noise
GUMBEL_SHAPES = [(1, 1, 1), (1, 5, 5), (3, 77, 8), (5, 1030, 41), (2, 70001, 4), (70, 515, 16), (4, 300, 256)]
GUMBEL_CASES = [(F, I, k, 7000 + n) for n, (F, I, k) in enumerate(GUMBEL_SHAPES)]


@functools.lru_cache(maxsize=None)
def gumbel_inputs(F, I, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(F, I, generator=g)
    noise = -torch.empty(k, F, I).exponential_(generator=g).log()
    dS = torch.randn(F, I, generator=g)
    return x, noise, dS


def gumbel_float64(x, noise, dS, k, tau):
    """(S, picks, smallest top-2 gap, dx) of the float64 restatement.  With a single item there is no runner-up (the restatement's top-2 needs two
    items): its one round is a softmax over one item, so S = 1, the pick is item 0 and dx = 0."""
    if x.shape[1] == 1:
        return torch.ones(x.shape, dtype=torch.float64), torch.zeros(x.shape[0], 1, dtype=torch.int64), float('inf'), torch.zeros(x.shape, dtype=torch.float64)
    x64 = x.double().requires_grad_()
    S, picks, gap = rs.gumbel_topk_relaxed(x64, k, noise.double(), tau=tau)
    S.backward(dS.double())
    return S.detach(), picks, gap, x64.grad


@pytest.mark.parametrize('tau', [1.0, 0.5])
@pytest.mark.parametrize('F,I,k,seed', GUMBEL_CASES)
def test_gumbel_topk_against_float64(F, I, k, seed, tau):
    from arlib_amd import ops
    from arlib_amd.attack.Black.GSPAttack import gumbel_topk_relaxed
    x, noise, dS = gumbel_inputs(F, I, k, seed)
    S64, picks64, gap, dx64 = gumbel_float64(x, noise, dS, k, tau)
    print('gumbel F=%d I=%d k=%d tau=%g: smallest float64 top-2 gap %.3e' % (F, I, k, tau, gap))
    assert gap >= 1e-4                                                          # no fp32 / fp64 near-tie can flip a pick

    def run(fn):
        xd = x.to(DEV).requires_grad_()
        S, picks = fn(xd, k, tau=tau, noise=noise.to(DEV))
        S.backward(dS.to(DEV))
        return S.detach(), picks, xd.grad
    S, picks, dx = run(ops.gumbel_topk)
    Sc, picks_c, dxc = run(gumbel_topk_relaxed)
    assert picks.dtype == torch.int64 and picks.shape == (F, k)
    assert torch.equal(picks.cpu(), picks64)
    what = 'gumbel F=%d I=%d k=%d tau=%g' % (F, I, k, tau)
    held(what, 'S', S, Sc, S64)
    held(what, 'dx', dx, dxc, dx64)
    held(what, 'rowsum', S.double().sum(1), Sc.double().sum(1), torch.full((F,), float(k), dtype=torch.float64))
    S2, picks2, dx2 = run(ops.gumbel_topk)
    assert torch.equal(S, S2) and torch.equal(picks, picks2) and torch.equal(dx, dx2)


def test_gumbel_topk_logsumexp_and_stats():
    from arlib_amd import ops
    F, I, k, seed = GUMBEL_CASES[3]
    x, noise, _ = gumbel_inputs(F, I, k, seed)
    S, picks, lse, stats = ops.gumbel_topk_fwd(x.to(DEV), k, tau=0.5, noise=noise.to(DEV))
    z = (x.double()[None] + noise.double()) / 0.5                              # [k, F, I]
    p = picks.cpu().long()
    for r in range(k):
        zr = z[r].clone()
        if r:
            zr.scatter_(1, p[:, :r], float('-inf'))
        assert rel(lse[:, r].cpu().numpy(), torch.logsumexp(zr, 1).numpy()) <= 1e-6
        assert rel(stats[:, r, 0].cpu().numpy(), zr.max(1)[0].numpy()) <= 1e-6
    assert rel(lse.cpu().numpy(), (stats[:, :, 0].double() + stats[:, :, 1].double().log()).cpu().numpy()) <= 1e-6


# ------------------------------------------------------------------------------------------------ hash noise
def test_hash_noise_is_a_function_of_its_five_numbers():
    from arlib_amd import ops
    a = ops.gumbel_noise(11, 0, 4, 8, 4096, DEV)
    assert a.shape == (4, 8, 4096) and a.dtype == torch.float32 and bool(torch.isfinite(a).all())
    assert torch.equal(a, ops.gumbel_noise(11, 0, 4, 8, 4096, DEV))
    assert not torch.equal(a, ops.gumbel_noise(11, 1, 4, 8, 4096, DEV)) and not torch.equal(a, ops.gumbel_noise(12, 0, 4, 8, 4096, DEV))
    big = ops.gumbel_noise(11, 0, 5, 10, 4101, DEV)
    assert bool(torch.isfinite(big).all()) and torch.equal(a, big[:4, :8, :4096])              # not a function of k, F or I
    sigma = (math.pi / math.sqrt(6.0)) / math.sqrt(4 * 8 * 4096)                               # the Gumbel law's deviation over 131 072 draws: 3.5e-3
    mean = float(a.double().mean())
    print('hash noise: mean %.5f (Euler gamma 0.57722), sigma of the mean %.2e' % (mean, sigma))
    assert abs(mean - 0.5772156649015329) <= 5 * sigma
    assert len(torch.unique(a)) > 65_536                                                       # 24-bit draws: mostly distinct among 131 072


@pytest.mark.parametrize('F,I,k', [(3, 77, 8), (5, 1030, 41)])
def test_hash_noise_in_the_kernels_is_the_tensor_draw(F, I, k):
    from arlib_amd import ops
    from arlib_amd.attack.Black.GSPAttack import gumbel_topk_relaxed
    g = torch.Generator().manual_seed(F + I)
    x, dS = torch.randn(F, I, generator=g).to(DEV), torch.randn(F, I, generator=g).to(DEV)
    seed, call = 1234567, 3

    def run(fn, **kw):
        xd = x.clone().requires_grad_()
        S, picks = fn(xd, k, **kw)
        S.backward(dS)
        return S.detach(), picks, xd.grad
    noise = ops.gumbel_noise(seed, call, k, F, I, DEV)
    by_seed, by_tensor = run(ops.gumbel_topk, seed=seed, call=call), run(ops.gumbel_topk, noise=noise)
    comp = run(gumbel_topk_relaxed, noise=noise)
    assert torch.equal(by_seed[1], by_tensor[1]) and torch.equal(by_seed[1], comp[1])
    # z = (x + g) / tau has the composed route's bits, so the picks agree whatever the draw's top-2 gap is; S and dx against the tensor call's
    for n, name in ((0, 'S'), (2, 'dx')):
        print('gumbel hash F=%d %s: seed against tensor %.3e, composed against tensor %.3e'
              % (F, name, rel(by_seed[n].cpu().numpy(), by_tensor[n].cpu().numpy()), rel(comp[n].cpu().numpy(), by_tensor[n].cpu().numpy())))
    assert rel(by_seed[0].cpu().numpy(), by_tensor[0].cpu().numpy()) <= FLOOR and rel(by_seed[2].cpu().numpy(), by_tensor[2].cpu().numpy()) <= FLOOR
    again = run(ops.gumbel_topk, seed=seed, call=call)
    assert all(torch.equal(a, b) for a, b in zip(by_seed, again))
    other = run(ops.gumbel_topk, seed=seed, call=call + 1)
    assert not torch.equal(other[0], by_seed[0])
    with pytest.raises(ValueError):
        ops.gumbel_topk(x, k)                                                                   # neither noise nor seed
    with pytest.raises(ValueError):
        ops.gumbel_topk(x, k, noise=noise, seed=seed)                                           # both


# ------------------------------------------------------------------------------------------------ upstream scaling and dispatch
def test_doubling_the_upstream_doubles_the_gradients_exactly():
    from arlib_amd import ops
    F, I, k, seed = GUMBEL_CASES[3]
    x, noise, dS = (t.to(DEV) for t in gumbel_inputs(F, I, k, seed))
    _, picks, _, stats = ops.gumbel_topk_fwd(x, k, noise=noise)
    one, two = ops.gumbel_topk_bwd(dS, x, k, picks, stats, noise=noise), ops.gumbel_topk_bwd(2 * dS, x, k, picks, stats, noise=noise)
    assert torch.equal(two, 2 * one) and float(one.abs().max()) > 0
    A, B, w2, b2, up, _ = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in pair_problem(5, 1030, 41, seed=3))
    for a, b in zip(ops.pair_mlp_bwd(up, A, B, w2, b2), ops.pair_mlp_bwd(2 * up, A, B, w2, b2)):
        assert torch.equal(b, 2 * a)


def test_past_the_limits_the_dispatchers_take_the_composed_routes(monkeypatch):
    from arlib_amd import ops, profilegen as pg
    from arlib_amd.attack.Black.GSPAttack import gumbel_topk_relaxed
    calls = []
    for name in ('pair_mlp_logits_composed', 'gumbel_topk_composed'):
        orig = getattr(pg, name)
        monkeypatch.setattr(pg, name, (lambda o, n: lambda *a, **k: calls.append(n) or o(*a, **k))(orig, name))
    g = torch.Generator().manual_seed(1)
    # inside the limits: the kernels
    A, B, w2, b2, _, _ = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in pair_problem(3, 77, 8, seed=2))
    x = torch.randn(2, 600, generator=g).to(DEV)
    noise = -torch.empty(513, 2, 600).exponential_(generator=g).log().to(DEV)
    ops.pair_mlp_logits_auto(A, B, w2, b2); ops.gumbel_topk_auto(x, 8, noise=noise[:8].contiguous())
    assert calls == []
    # H above PAIR_MLP_MAX_H
    H = pg.PAIR_MLP_MAX_H + 1
    A, B, w2, b2, up, _ = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in pair_problem(2, 50, H, seed=4))
    assert not ops.pair_mlp_supported(2, 50, H)
    with pytest.raises(ValueError):
        ops.pair_mlp_logits(A, B, w2, b2)
    got = ops.pair_mlp_logits_auto(A, B, w2, b2)
    assert calls == ['pair_mlp_logits_composed']
    want = pair_float64(A.cpu(), B.cpu(), w2.cpu(), b2.cpu(), up.cpu())[0]
    assert rel(got.cpu().numpy(), want.numpy()) <= 1e-5
    # k above GUMBEL_MAX_K
    k = pg.GUMBEL_MAX_K + 1
    assert not ops.gumbel_topk_supported(2, 600, k)
    with pytest.raises(ValueError):
        ops.gumbel_topk(x, k, noise=noise)
    S, picks = ops.gumbel_topk_auto(x, k, noise=noise)
    assert calls == ['pair_mlp_logits_composed', 'gumbel_topk_composed']
    Sc, picks_c = gumbel_topk_relaxed(x, k, noise=noise)
    assert torch.equal(S, Sc) and torch.equal(picks, picks_c)
    # a smaller limit sends a shape the kernels take to the composed route, and the two agree
    monkeypatch.setattr(pg, 'GUMBEL_MAX_K', 4)
    S8, picks8 = ops.gumbel_topk_auto(x, 8, noise=noise[:8].contiguous())
    monkeypatch.setattr(pg, 'GUMBEL_MAX_K', 512)
    Sk, picks_k = ops.gumbel_topk_auto(x, 8, noise=noise[:8].contiguous())
    assert calls[-1] == 'gumbel_topk_composed' and len(calls) == 3
    assert torch.equal(picks8, picks_k) and rel(S8.cpu().numpy(), Sk.cpu().numpy()) <= 1e-5


# ------------------------------------------------------------------------------------------------ the attack on the fused route
def fused_route(monkeypatch, noise_source='torch'):
    """run_device_attack builds the attack itself: set the route on the instance at the top of posionDataAttack."""
    from arlib_amd.attack.Black.GSPAttack import GSPAttack
    orig = GSPAttack.posionDataAttack

    def run(self):
        self.profile_route, self.noise_source = 'fused', noise_source
        return orig(self)
    monkeypatch.setattr(GSPAttack, 'posionDataAttack', run)


def test_one_fused_attack_against_float64(monkeypatch):
    """Exactly the assertions of test_gpu_gsp.py::test_one_attack_against_float64, on the fused route."""
    fused_route(monkeypatch)
    data, args, params, noises = attack_problem()
    atk, before, res = run_device_attack(data, args, params, noises)
    assert atk.profile_route == 'fused' and atk.noise_source == 'torch'
    want = restated_attack(before, atk.targetItem, atk.maliciousFeedbackNum, params, noises)
    U, F, I, k, T = 300, 4, 120, 6, 2
    print('fused gsp attack: smallest top-2 gap %.3e, losses %s (float64 %s)' % (want['gap'], atk.loss_log, want['loss']))
    assert want['gap'] >= 1e-3
    assert len(atk.pick_log) == 3 and all(torch.equal(a, b) for a, b in zip(atk.pick_log, want['picks']))
    assert len(atk.loss_log) == 3 and close(np.asarray(atk.loss_log), np.asarray(want['loss']))
    assert close(atk.first_dS.cpu().numpy(), want['dS'].numpy())
    assert res.shape == (U + F, I) == atk.interact.shape and (res[:U] != before).nnz == 0
    fake = np.asarray(res[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0}
    assert (fake[:, atk.targetItem] == 1).all() and ((fake.sum(1) >= k) & (fake.sum(1) <= k + T)).all()
    assert atk.fakeUser == list(range(U, U + F))


class _NeverDrawn:
    def to(self, device):
        raise AssertionError('the hash route called _noise')


def test_fused_attack_with_hash_noise(monkeypatch):
    fused_route(monkeypatch, 'hash')
    U, F, I, k, T = 300, 4, 120, 6, 2

    def run():
        data, args, params, _ = attack_problem()
        atk, before, res = run_device_attack(data, args, params, [_NeverDrawn()])
        return atk, before, res
    atk, before, res = run()
    assert atk.noise_source == 'hash' and len(atk.loss_log) == 3 and all(np.isfinite(atk.loss_log))
    assert len(atk.pick_log) == 3 and all(p.shape == (F, k) and all(len(set(row)) == k for row in p.tolist()) for p in atk.pick_log)
    assert not torch.equal(atk.pick_log[0], atk.pick_log[1])                                  # the epoch number is the hash's call
    assert res.shape == (U + F, I) and (res[:U] != before).nnz == 0
    fake = np.asarray(res[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0}
    assert (fake[:, atk.targetItem] == 1).all() and ((fake.sum(1) >= k) & (fake.sum(1) <= k + T)).all()
    atk2, _, res2 = run()                                                                     # run_device_attack seeds Python's random itself
    assert atk2.loss_log == atk.loss_log and all(torch.equal(a, b) for a, b in zip(atk.pick_log, atk2.pick_log))
    assert torch.equal(atk.first_dS, atk2.first_dS) and (res != res2).nnz == 0

"""Poisoned scratch memory (tests/poison.py) for GSPAttack's profile generator: the pair-MLP and Gumbel top-k kernels write every output and
workspace word before they read it (the picked items' bitmask is cleared by the kernel that uses it), so a call on NaN-filled allocations gives the
bits of a clean call; so does one attack epoch on the fused route."""
import inspect

import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected
from test_gpu_gsp import attack_problem, run_device_attack
from test_gpu_profilegen import pair_problem, fused_route

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(3, 77, 8), (5, 1030, 41)]                                  # (F, I, H = k)
SEED, CALL = 99, 2


def inputs(F, I, n):
    A, B, w2, b2, up, _ = pair_problem(F, I, n, seed=F)
    g = torch.Generator().manual_seed(I)
    x = torch.randn(F, I, generator=g)
    noise = -torch.empty(n, F, I).exponential_(generator=g).log()
    return dict(A=A.to(DEV), B=B.to(DEV), w2=w2.to(DEV), b2=b2.to(DEV), up=up.to(DEV), x=x.to(DEV), noise=noise.to(DEV), k=n)


def _autograd(fn, leaves, up):
    leaves = [t.clone().requires_grad_() for t in leaves]
    out = fn(*leaves)
    first = out[0] if isinstance(out, tuple) else out
    first.backward(up)
    return [out] + [t.grad for t in leaves]


def _gumbel_bwd(pg, P, **src):
    _, picks, _, stats = pg.gumbel_topk_fwd(P['x'], P['k'], tau=0.5, **src)
    return pg.gumbel_topk_bwd(P['up'], P['x'], P['k'], picks, stats, tau=0.5, **src)


# name -> (call without gradient, call with gradient); the raw kernel wrappers have one form
CASES = {
    'pair_mlp_fwd': lambda pg, P, g: pg.pair_mlp_fwd(P['A'], P['B'], P['w2'], P['b2']),
    'pair_mlp_bwd': lambda pg, P, g: pg.pair_mlp_bwd(P['up'], P['A'], P['B'], P['w2'], P['b2']),
    'pair_mlp_logits': lambda pg, P, g: (_autograd(pg.pair_mlp_logits, [P['A'], P['B'], P['w2'], P['b2']], P['up']) if g
                                         else pg.pair_mlp_logits(P['A'], P['B'], P['w2'], P['b2'])),
    'gumbel_noise': lambda pg, P, g: pg.gumbel_noise(SEED, CALL, P['k'], P['x'].shape[0], P['x'].shape[1], DEV),
    'gumbel_topk_fwd': lambda pg, P, g: pg.gumbel_topk_fwd(P['x'], P['k'], tau=0.5, **(dict(seed=SEED, call=CALL) if g else dict(noise=P['noise']))),
    'gumbel_topk_bwd': lambda pg, P, g: _gumbel_bwd(pg, P, **(dict(seed=SEED, call=CALL) if g else dict(noise=P['noise']))),
    'gumbel_topk': lambda pg, P, g: (_autograd(lambda x: pg.gumbel_topk(x, P['k'], noise=P['noise']), [P['x']], P['up']) if g
                                     else pg.gumbel_topk(P['x'], P['k'], noise=P['noise'])),
    'gumbel_topk_hash': lambda pg, P, g: (_autograd(lambda x: pg.gumbel_topk(x, P['k'], seed=SEED, call=CALL), [P['x']], P['up']) if g
                                          else pg.gumbel_topk(P['x'], P['k'], seed=SEED, call=CALL)),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import profilegen as pg
    found = introspected(inspect.getsource(pg))
    assert {'pair_mlp_fwd', 'pair_mlp_bwd', 'gumbel_topk_fwd', 'gumbel_topk_bwd', 'gumbel_noise'} <= found      # the introspection sees the wrappers' torch.empty
    assert sorted(found - set(CASES)) == []
    assert all(hasattr(pg, n) for n in CASES if n != 'gumbel_topk_hash')


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('F,I,n', SHAPES)
@pytest.mark.parametrize('grad', [False, True])
def test_op_is_independent_of_scratch_memory(name, F, I, n, grad):
    from arlib_amd import profilegen as pg
    P = inputs(F, I, n)
    clean = CASES[name](pg, P, grad)
    with poison.poisoned_allocations():
        dirty = CASES[name](pg, P, grad)
    assert poison.compare(clean, dirty) == []                           # fixed-order reductions: the same bits
    assert not poison.has_nan(dirty)


def test_workspace_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks (a larger row's bitmask, more splits): results equal a fresh process's."""
    from arlib_amd import profilegen as pg
    big, small = inputs(5, 1030, 41), inputs(3, 77, 8)

    def run(P):
        return (CASES['pair_mlp_bwd'](pg, P, True), CASES['gumbel_topk'](pg, P, True))
    torch.cuda.empty_cache()
    alone = run(small)
    run(big)
    assert poison.compare(alone, run(small)) == []


def test_one_fused_attack_epoch_is_independent_of_scratch_memory(monkeypatch):
    fused_route(monkeypatch)

    def epoch():
        data, args, params, noises = attack_problem(epochs=1)
        atk, _, res = run_device_attack(data, args, params, noises)
        assert atk.profile_route == 'fused'
        return dict(loss=atk.loss_log, dS=atk.first_dS, picks=atk.pick_log, fake=res[300:].toarray(),
                    tables=[p.detach().clone() for p in atk.ngcf.parameters()])
    clean = epoch()
    with poison.poisoned_allocations():
        dirty = epoch()
    assert poison.compare(clean, dirty) == []
    assert not poison.has_nan(dirty)

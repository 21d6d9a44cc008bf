"""Poisoned scratch memory (tests/poison.py) for PoisonRec's policy head: the kernels write every output and workspace word before they read it (the
packed actions included: every word of a row has one writer), so a call on NaN-filled allocations gives the bits of a clean call, and a workspace
reused between a large and a small shape leaves the small shape's results unchanged."""
import inspect

import pytest
import torch
import poison
import stream_splits_restatement as splits
from test_gpu_poisoned_memory import introspected
from test_gpu_policyhead import on_device

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLIT = splits.BOTH_SPLIT_SHAPE                                        # part_ms, part_sum, part_dq and part_dE with more than one split each
SHAPES = [(3, 77, 16), (70, 4099, 64), SPLIT]
SEED, CALL = 99, 2


def inputs(B, I, d):
    q, E, words, gl, ge, u = on_device(B, I, d, 'plain')
    return dict(q=q, E=E, words=words, gl=gl, ge=ge, u=u, B=B, I=I)


def _autograd(ph, P, route):
    q, E = P['q'].clone().requires_grad_(), P['E'].clone().requires_grad_()
    logp, ent = ph.bernoulli_softmax_head(q, E, P['words'], route=route)
    (P['gl'] * logp + P['ge'] * ent).sum().backward()
    return [logp.detach(), ent.detach(), q.grad, E.grad]


# name -> call(module, problem, with gradients / with the hash)
CASES = {
    'bernoulli_softmax_eval': lambda ph, P, g: ph.bernoulli_softmax_eval(P['q'], P['E'], P['words'], P['gl'], P['ge'], want_grad=g),
    'bernoulli_softmax_eval_composed': lambda ph, P, g: ph.bernoulli_softmax_eval_composed(P['q'], P['E'], P['words'], P['gl'], P['ge'], want_grad=g),
    'bernoulli_softmax': lambda ph, P, g: ph.bernoulli_softmax(P['q'], P['E'], P['words'], P['gl'], P['ge'], want_grad=g),
    'bernoulli_softmax_head': lambda ph, P, g: _autograd(ph, P, 'fused' if g else 'composed'),
    'bernoulli_uniforms': lambda ph, P, g: ph.bernoulli_uniforms(SEED, CALL, P['B'], P['I'], row0=3 if g else 0, device=DEV),
    'bernoulli_softmax_sample': lambda ph, P, g: ph.bernoulli_softmax_sample(P['q'], P['E'], **(dict(seed=SEED, call=CALL) if g else dict(u=P['u']))),
    'bernoulli_softmax_sample_deterministic': lambda ph, P, g: ph.bernoulli_softmax_sample(P['q'], P['E'], deterministic=True),
    'bernoulli_softmax_sample_composed': lambda ph, P, g: ph.bernoulli_softmax_sample_composed(P['q'], P['E'], **(dict(seed=SEED, call=CALL) if g else dict(u=P['u']))),
    'bernoulli_softmax_sample_auto': lambda ph, P, g: ph.bernoulli_softmax_sample_auto(P['q'], P['E'], **(dict(seed=SEED, call=CALL) if g else dict(u=P['u']))),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import policyhead as ph
    found = introspected(inspect.getsource(ph))
    assert {'bernoulli_softmax_eval', 'bernoulli_softmax_sample', 'bernoulli_uniforms', 'bernoulli_softmax_eval_composed'} <= found
    assert sorted(found - set(CASES)) == []
    assert all(hasattr(ph, n) for n in CASES if n != 'bernoulli_softmax_sample_deterministic')


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('B,I,d', SHAPES)
@pytest.mark.parametrize('grad', [False, True])
def test_op_is_independent_of_scratch_memory(name, B, I, d, grad):
    from arlib_amd import policyhead as ph
    assert (splits.stage_splits(I, B)[0] > 1) == ((B, I, d) == SPLIT) and (splits.ph_item_splits(I)[0] > 1) == (I > 1024)
    P = inputs(B, I, d)
    clean = CASES[name](ph, P, grad)
    with poison.poisoned_allocations():
        dirty = CASES[name](ph, P, grad)
    assert poison.compare(clean, dirty) == []                           # fixed-order reductions: the same bits
    assert not poison.has_nan(dirty)


def test_workspace_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks (more splits, more action words): results equal a fresh process's."""
    from arlib_amd import policyhead as ph
    big, split, small = inputs(70, 4099, 64), inputs(*SPLIT), inputs(3, 77, 16)
    assert splits.ph_item_splits(SPLIT[1])[0] == splits.stage_splits(SPLIT[0], SPLIT[1])[0] == 3 and splits.stage_splits(SPLIT[1], SPLIT[0])[0] == 2

    def run(P):
        return (CASES['bernoulli_softmax_eval'](ph, P, True), CASES['bernoulli_softmax_sample'](ph, P, True), CASES['bernoulli_softmax_sample'](ph, P, False))
    torch.cuda.empty_cache()
    alone = run(small)
    run(big)
    run(split)
    assert poison.compare(alone, run(small)) == []

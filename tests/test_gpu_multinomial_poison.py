"""Poisoned scratch memory (tests/poison.py) for the multinomial likelihood: the kernels write every output and workspace word before they read it,
so a call on NaN-filled allocations gives the bits of a clean call, and a workspace reused between a large and a small shape leaves the small
shape's results unchanged."""
import inspect

import pytest
import torch
import poison
import stream_splits_restatement as splits
from test_gpu_poisoned_memory import introspected
from test_gpu_multinomial import on_device

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SPLIT = splits.BOTH_SPLIT_SHAPE                                        # part_ms, part_dq and part_dE with more than one split each
SHAPES = [(3, 77, 16), (70, 515, 64), SPLIT]


def inputs(B, I, d, weighted=True):
    q, E, P, g = on_device(B, I, d, 'plain', weighted)
    return dict(q=q, E=E, P=P, g=g)


def _autograd(mn, P, route):
    q, E = P['q'].clone().requires_grad_(), P['E'].clone().requires_grad_()
    nll = mn.multinomial_nll(q, E, P['P'], route=route)
    (P['g'] * nll).sum().backward()
    return [nll.detach(), q.grad, E.grad]


# name -> call(module, problem, with gradients)
CASES = {
    'multinomial_softmax_kernel': lambda mn, P, g: mn.multinomial_softmax_kernel(P['q'], P['E'], P['P'], P['g'], want_grad=g),
    'multinomial_softmax_composed': lambda mn, P, g: mn.multinomial_softmax_composed(P['q'], P['E'], P['P'], P['g'], want_grad=g),
    'multinomial_softmax': lambda mn, P, g: mn.multinomial_softmax(P['q'], P['E'], P['P'], P['g'], want_grad=g),
    'multinomial_nll': lambda mn, P, g: _autograd(mn, P, 'fused' if g else 'composed'),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import multinomial as mn
    found = introspected(inspect.getsource(mn))
    assert {'multinomial_softmax_kernel', 'multinomial_softmax_composed'} <= found
    assert sorted(found - set(CASES)) == []
    assert all(hasattr(mn, n) for n in CASES)


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('B,I,d', SHAPES)
@pytest.mark.parametrize('grad', [False, True])
def test_op_is_independent_of_scratch_memory(name, B, I, d, grad):
    from arlib_amd import multinomial as mn
    assert (min(splits.stage_splits(B, I)[0], splits.stage_splits(I, B)[0]) > 1) == ((B, I, d) == SPLIT)
    for weighted in (False, True):
        P = inputs(B, I, d, weighted)
        clean = CASES[name](mn, P, grad)
        with poison.poisoned_allocations():
            dirty = CASES[name](mn, P, grad)
        assert poison.compare(clean, dirty) == []                       # fixed-order reductions: the same bits
        assert not poison.has_nan(dirty)


def test_workspace_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks (more splits, wider rows): results equal a fresh process's."""
    from arlib_amd import multinomial as mn
    big, split, small = inputs(70, 515, 64), inputs(*SPLIT), inputs(3, 77, 16)
    assert splits.stage_splits(SPLIT[0], SPLIT[1])[0] == 3 and splits.stage_splits(SPLIT[1], SPLIT[0])[0] == 2

    def run(P):
        return (CASES['multinomial_softmax_kernel'](mn, P, True), CASES['multinomial_softmax_kernel'](mn, P, False))
    torch.cuda.empty_cache()
    alone = run(small)
    run(big)
    run(split)
    assert poison.compare(alone, run(small)) == []

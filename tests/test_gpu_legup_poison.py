"""Poisoned scratch memory (tests/poison.py) for the ranking-loss ops of arlib_amd/colsoftmax.py: every workspace word is written before it is read,
so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies
the same introspection to the module these ops live in."""
import inspect

import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def problem(U, I, d, T, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(U, d, generator=g) * 0.15).to(DEV), (torch.randn(I, d, generator=g) * 0.15).to(DEV), torch.randperm(I, generator=g)[:T].tolist()


# (U, I, d, T): three splits of the streamed users with a ragged last one / one split, ragged tiles, the widest rows
SHAPES = [(9001, 333, 64, 5), (130, 77, 16, 1), (2049, 515, 128, 5)]
CASES = {
    'colsoftmax_target_loss': lambda cs, P, g: cs.colsoftmax_target_loss(*P, want_grad=g),
    'colsoftmax_target_loss_composed': lambda cs, P, g: cs.colsoftmax_target_loss_composed(*P, want_grad=g),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import colsoftmax as cs
    found = introspected(inspect.getsource(cs))
    assert 'colsoftmax_target_loss' in found                            # the introspection sees the kernel wrapper's torch.empty
    assert sorted(found - set(CASES)) == []


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('U,I,d,T', SHAPES)
@pytest.mark.parametrize('grad', [False, True])
def test_op_is_independent_of_scratch_memory(name, U, I, d, T, grad):
    from arlib_amd import colsoftmax as cs
    P = problem(U, I, d, T, seed=U)
    clean = CASES[name](cs, P, grad)
    with poison.poisoned_allocations():
        dirty = CASES[name](cs, P, grad)
    if name == 'colsoftmax_target_loss':
        assert poison.compare(clean, dirty) == []                       # fixed-order reductions: the same bits
    else:
        for a, b in zip(clean, dirty):                                  # torch's own reductions may reorder: the same values to fp32 rounding
            torch.testing.assert_close(a, b, rtol=1e-5, atol=0)
    assert not poison.has_nan(dirty)


def test_workspace_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import colsoftmax as cs
    big, small = problem(9001, 333, 64, 5, seed=1), problem(700, 333, 64, 5, seed=2)
    torch.cuda.empty_cache()
    alone = cs.colsoftmax_target_loss(*small, want_grad=True)
    cs.colsoftmax_target_loss(*big, want_grad=True)
    after = cs.colsoftmax_target_loss(*small, want_grad=True)
    assert poison.compare(alone, after) == []

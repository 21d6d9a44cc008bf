"""Poisoned scratch memory (tests/poison.py) for the target-rank op: the kernel and the composed route of arlib_amd/targetrank.py write every workspace
and output word before they read it, so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads
arlib_amd/ops.py; this file applies the same introspection to the module the op lives in (the pattern of test_gpu_apr_poison.py)."""
import inspect

import pytest
import torch
import poison
import rank_restatement as R
from test_gpu_poisoned_memory import introspected
from test_targetrank_cpu import case, tens

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [1, 2, 4]             # one block, one target group; three blocks, T = 17; a split item stream (integer partials in the workspace), T = 64


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import targetrank
    assert introspected(inspect.getsource(targetrank)) == {'target_rank_kernel', 'target_rank_composed'}
    public = {n for n, f in vars(targetrank).items() if inspect.isfunction(f) and f.__module__ == targetrank.__name__ and not n.startswith('_')}
    # target_rank_supported is host-only (a shape test); target_rank only hands its arguments to one of the two routes below
    assert public == {'target_rank_kernel', 'target_rank_composed', 'target_rank_supported', 'target_rank'}


def _run(route, k, masked):
    from arlib_amd import targetrank
    Pu, Pi, targets, mask, _ = case(k, masked)
    fn = {'kernel': targetrank.target_rank_kernel, 'composed': targetrank.target_rank_composed, 'dispatcher': targetrank.target_rank}[route]
    return fn(tens(Pu, DEV), tens(Pi, DEV), tens(targets, DEV), (tens(mask[0], DEV), tens(mask[1], DEV)) if masked else None)


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('route', ['kernel', 'composed', 'dispatcher'])
@pytest.mark.parametrize('k', SHAPES, ids=[R.IDS[k] for k in SHAPES])
def test_route_is_independent_of_scratch_memory(k, route, masked):
    from arlib_amd import _lib
    if k == 4:
        U, I, T, d, _ = R.CASES[k]
        assert _lib.lib().arl_target_rank_workspace_bytes(U, I, d, T) > 0             # the case does go through the workspace
    clean = _run(route, k, masked)
    with poison.poisoned_allocations():
        dirty = _run(route, k, masked)
        again = _run(route, k, masked)                                               # the caching allocator hands the poisoned blocks back
    assert poison.compare(clean, dirty) == [] and poison.compare(clean, again) == []
    assert not poison.has_nan(dirty) and not poison.has_nan(again)
    assert bool((dirty[0] >= -1).all())                                              # no -1 fill left in the counts either (ranks start at -1 only where listed)
    assert bool(((dirty[0] == -1).sum() == 0) or masked)

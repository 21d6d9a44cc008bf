"""Poisoned scratch memory (tests/poison.py) for the ops of arlib_amd/pairloss.py: every output and workspace word is written before it is read, so
a run on NaN-filled allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies
the same introspection to the module these ops live in (the pattern of test_gpu_kmeans_poison.py)."""
import inspect

import pytest
import torch
import poison
from conftest import golden
from test_gpu_poisoned_memory import introspected
from test_pairloss_cpu import unif_sets, unif_input

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G33 = golden('g33_pairloss.npz')
SHAPES = sorted(unif_sets(G33)[5:], key=lambda s: s[1])[:3]              # the three smallest shapes, on the clustered rows (duplicate and zero row included)


def problem(name):
    x = torch.from_numpy(unif_input(G33, name)).to(DEV)
    return x, x.flip(0).contiguous() * 0.5 + 0.25


CASES = {
    'uniformity': lambda pl, x, y: pl.uniformity(x),
    'uniformity_forward_only': lambda pl, x, y: pl.uniformity(x, want_grad=False),
    'uniformity_upstream': lambda pl, x, y: pl.uniformity(y, t=0.5, upstream=-3.0),
    'alignment': lambda pl, x, y: pl.alignment(x, y),
    'alignment_alpha1_forward_only': lambda pl, x, y: pl.alignment(x, y, alpha=1, want_grad=False),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import pairloss
    found = introspected(inspect.getsource(pairloss))
    assert found == {'uniformity', 'alignment'}                             # the introspection sees the kernel wrappers' torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(pairloss).items() if inspect.isfunction(f) and f.__module__ == pairloss.__name__ and not n.startswith('_')}
    assert public - set(CASES) == {'uniformity_splits'}                     # host-only: a count, no device memory


@pytest.mark.parametrize('case', sorted(CASES))
@pytest.mark.parametrize('name,n,d', SHAPES, ids=[s[0] for s in SHAPES])
def test_op_is_independent_of_scratch_memory(case, name, n, d):
    from arlib_amd import pairloss
    P = problem(name)
    clean = CASES[case](pairloss, *P)
    with poison.poisoned_allocations():
        dirty = CASES[case](pairloss, *P)
    assert poison.compare(clean, dirty) == []                               # fixed-order reductions: the same bits
    assert not poison.has_nan(dirty)


def test_workspace_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import pairloss
    big, small = problem('unif_clust_1061x128')[0], problem('unif_clust_130x64')[0]
    small128 = big[:130].contiguous()
    torch.cuda.empty_cache()
    alone = (pairloss.uniformity(small), pairloss.uniformity(small128), pairloss.alignment(small, small.flip(0).contiguous()))
    pairloss.uniformity(big); pairloss.alignment(big, big.flip(0).contiguous())
    after = (pairloss.uniformity(small), pairloss.uniformity(small128), pairloss.alignment(small, small.flip(0).contiguous()))
    assert poison.compare(alone, after) == []

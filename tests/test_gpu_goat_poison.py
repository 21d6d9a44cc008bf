"""Poisoned scratch memory (tests/poison.py) for the co-rating op of arlib_amd/corating.py: the output and the item-major index are written before
they are read, and the kernel's bitmap lives in LDS, so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of
test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies the same introspection to the module this op lives in."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import poison
from test_gpu_poisoned_memory import introspected

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def problem(I, seed):
    """U 200 x I interactions with a hub item, an item nobody rated (its output word is written without the bitmap) and a user without items."""
    rng = np.random.RandomState(seed)
    D = rng.random_sample((200, I)) < min(0.05, 40.0 / I)
    D[:, I // 2] = True
    D[:, I - 2] = False
    D[17] = False
    X = sp.csr_matrix(D.astype(np.float32))
    return X.indptr.astype(np.int64), X.indices.astype(np.int32), 200, I


def _device_inputs(co, rp, col, U, I):
    return co.corating_degree(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), U, I)


# one ragged word above the first / the ml-100k catalogue / several clear passes per thread and a ragged last word
SIZES = [33, 1412, 4099]
CASES = {
    'corating_degree': lambda co, rp, col, U, I: co.corating_degree(rp, col, U, I),
    'corating_degree_device_inputs': _device_inputs,
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import corating
    found = introspected(inspect.getsource(corating))
    assert 'corating_degree' in found                                       # the introspection sees the kernel wrapper's torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(corating).items() if inspect.isfunction(f) and f.__module__ == corating.__name__ and not n.startswith('_')}
    assert public - set(CASES) == {'corating_degree_supported', 'corating_degree_host'}        # host-only: a comparison, and scipy's product


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('I', SIZES)
def test_op_is_independent_of_scratch_memory(name, I):
    from arlib_amd import corating
    P = problem(I, seed=I)
    clean = CASES[name](corating, *P)
    with poison.poisoned_allocations():
        dirty = CASES[name](corating, *P)
    assert poison.compare(clean, dirty) == []                               # an integer result: the same bits
    assert int(clean[I - 2]) == 0 and int(clean[I // 2]) == int((clean > 0).sum())
    assert np.array_equal(clean.cpu().numpy(), corating.corating_degree_host(sp.csr_matrix((np.ones(len(P[1])), P[1], P[0]), shape=(200, I))))


def test_output_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import corating
    big, small = problem(4099, 1), problem(1412, 2)
    torch.cuda.empty_cache()
    alone = corating.corating_degree(*small)
    corating.corating_degree(*big)
    after = corating.corating_degree(*small)
    assert poison.compare(alone, after) == []

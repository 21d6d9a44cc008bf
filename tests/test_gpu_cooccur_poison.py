"""Poisoned scratch memory (tests/poison.py) for the neighbour op of arlib_amd/neighbours.py: both outputs are written in full by the kernel (the
padding included), the canonical CSR, the column-major index and the launch order are written before they are read, and the kernel's counters,
list, pending buffer and cursors live in LDS and are written before they are read, so a run on poisoned allocations gives the bits of a clean
run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies the same introspection to the module this op lives in."""
import inspect

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import poison
from test_gpu_poisoned_memory import introspected

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TILE = 64


def problem(n, seed):
    """n x 90 interactions with a hub column, a column nobody has, an empty row (its output is padding only) and a row alone on its column."""
    rng = np.random.RandomState(seed)
    D = rng.random_sample((n, 90)) < 0.06
    D[:, 40] = True
    D[:, 88:] = False
    D[n // 2] = False
    D[n - 1] = False
    D[n - 1, 89] = True
    X = sp.csr_matrix(D.astype(np.int64))
    return X.indptr.astype(np.int64), X.indices.astype(np.int32), n, 90


def _device_inputs(nb, rp, col, n, I, **kw):
    return nb.cooccur_topk(torch.from_numpy(rp).to(DEV), torch.from_numpy(col).to(DEV), n, I, 12, 'cosine', tile_rows=TILE, route='kernel', **kw)


def _rows(nb, rp, col, n, I):
    return _device_inputs(nb, rp, col, n, I, rows=torch.tensor([n - 1, 0, n // 2, 3, 0]))


# one tile / several whole tiles / whole tiles and a ragged one
SIZES = [50, 4 * TILE, 3 * TILE + 21]
CASES = {
    'cooccur_topk': lambda nb, rp, col, n, I: nb.cooccur_topk(rp, col, n, I, 12, 'jaccard', tile_rows=TILE, device=DEV, route='kernel'),
    'cooccur_topk_device_inputs': _device_inputs,
    'cooccur_topk_rows': _rows,
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import neighbours
    found = introspected(inspect.getsource(neighbours))
    assert 'cooccur_topk' in found                                          # the introspection sees the kernel wrapper's torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(neighbours).items() if inspect.isfunction(f) and f.__module__ == neighbours.__name__ and not n.startswith('_')}
    # host-only: a comparison of sizes, scipy's product, numpy arithmetic on the returned integers
    assert public - set(CASES) == {'cooccur_supported', 'cooccur_topk_host', 'binary_csr', 'similarity'}


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('n', SIZES)
def test_op_is_independent_of_scratch_memory(name, n):
    from arlib_amd import neighbours
    P = problem(n, seed=n)
    clean = CASES[name](neighbours, *P)
    with poison.poisoned_allocations():
        dirty = CASES[name](neighbours, *P)
    assert poison.compare(clean, dirty) == []                               # an integer result: the same bits
    X = sp.csr_matrix((np.ones(len(P[1]), np.int64), P[1], P[0]), shape=(n, 90))
    rows = [n - 1, 0, n // 2, 3, 0] if name == 'cooccur_topk_rows' else None
    ref = neighbours.cooccur_topk_host(X, 12, 'jaccard' if name == 'cooccur_topk' else 'cosine', rows)
    assert all(np.array_equal(c.cpu().numpy(), r) for c, r in zip(clean, ref))
    empty = [0, 2] if rows else [n - 1, n // 2]
    assert bool((clean[0][empty] == -1).all()) and bool((clean[1][empty] == 0).all())


def test_output_buffers_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import neighbours
    big, small = problem(4 * TILE, 1), problem(50, 2)
    torch.cuda.empty_cache()
    alone = CASES['cooccur_topk'](neighbours, *small)
    CASES['cooccur_topk'](neighbours, *big)
    after = CASES['cooccur_topk'](neighbours, *small)
    assert poison.compare(alone, after) == []

"""Poisoned scratch memory (tests/poison.py) for the scoring op of arlib_amd/userknn.py: the three outputs are written in full by the kernel (the
padding and the -1 ranks included), the canonical CSR, the sorted targets and the launch order are written before they are read, and the kernel's
accumulators, cursors, list, pending buffer and target counters live in LDS and are written before they are read, so a run on poisoned
allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file applies the same
introspection to the module this op lives in, as test_gpu_itemknn_poison.py does for arlib_amd/itemknn.py."""
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
USERS = 40
ROWS = [USERS - 1, 0, USERS // 2, 3, 0]


def problem(I, seed):
    """40 users x I items with a hub item, an item nobody has, an empty profile and a profile holding every item; user-side lists of 6 slots with
    unused ones, a repeated neighbour, the empty and the full user among the neighbours and weights up to 2^31 - 1; four targets, the last item
    among them."""
    rng = np.random.RandomState(seed)
    D = rng.random_sample((USERS, I)) < 0.1
    D[:, 7] = True
    D[:, I - 2] = False
    D[USERS // 2] = False
    D[USERS - 1] = True
    X = sp.csr_matrix(D.astype(np.int64))
    ni = rng.randint(-1, USERS, (USERS, 6)).astype(np.int32)
    ni[:, 4] = ni[:, 1]
    ni[::3, 2] = USERS - 1
    ni[1::3, 2] = USERS // 2
    nw = rng.randint(0, 2 ** 31 - 1, (USERS, 6)).astype(np.int32)
    return X.indptr.astype(np.int64), X.indices.astype(np.int32), I, ni, nw, [I - 1, 7, 0, I // 2]


def _device_inputs(kn, rp, col, I, ni, nw, tg, **kw):
    t = lambda a: torch.from_numpy(a).to(DEV)
    return kn.uknn_score_topk(t(rp), t(col), USERS, I, t(ni), t(nw), 12, mask_profile=True, targets=torch.tensor(tg).to(DEV), tile_items=TILE,
                              route='kernel', **kw)


def _rows(kn, rp, col, I, ni, nw, tg):
    return _device_inputs(kn, rp, col, I, ni, nw, tg, rows=torch.tensor(ROWS))


# one tile / several whole tiles / whole tiles and a ragged one
SIZES = [50, 4 * TILE, 3 * TILE + 21]
CASES = {
    'uknn_score_topk': lambda kn, rp, col, I, ni, nw, tg: kn.uknn_score_topk(rp, col, USERS, I, ni, nw, 12, targets=tg, tile_items=TILE, device=DEV, route='kernel'),
    'uknn_score_topk_device_inputs': _device_inputs,
    'uknn_score_topk_rows': _rows,
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import userknn
    found = introspected(inspect.getsource(userknn))
    assert 'uknn_score_topk' in found                                       # the introspection sees the kernel wrapper's torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(userknn).items() if inspect.isfunction(f) and f.__module__ == userknn.__name__ and not n.startswith('_')}
    # host-only: a comparison of sizes, numpy arithmetic on the lists, scipy's product
    assert public - set(CASES) == {'uknn_supported', 'weight_matrix', 'uknn_score_topk_host'}


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('I', SIZES)
def test_op_is_independent_of_scratch_memory(name, I):
    from arlib_amd import userknn
    P = problem(I, seed=I)
    clean = CASES[name](userknn, *P)
    with poison.poisoned_allocations():
        dirty = CASES[name](userknn, *P)
    assert poison.compare(clean, dirty) == []                               # an integer result: the same bits
    rp, col, _, ni, nw, tg = P
    X = sp.csr_matrix((np.ones(len(col), np.int64), col, rp), shape=(USERS, I))
    rows = ROWS if name == 'uknn_score_topk_rows' else None
    mask = name != 'uknn_score_topk'
    ref = userknn.uknn_score_topk_host(X, ni, nw, 12, rows, mask, tg)
    assert all(np.array_equal(c.cpu().numpy(), r) for c, r in zip(clean, ref))
    full = [0] if rows else [USERS - 1]
    if mask:                                                                # the profile holding every item: padding only, every rank -1
        assert bool((clean[0][full] == -1).all()) and bool((clean[1][full] == 0).all()) and bool((clean[2][full] == -1).all())
    else:                                                                   # every item is a candidate: the list is full
        assert bool((clean[0] >= 0).all()) and bool((clean[2] >= 0).all())


def test_output_buffers_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import userknn
    big, small = problem(4 * TILE, 1), problem(50, 2)
    torch.cuda.empty_cache()
    alone = CASES['uknn_score_topk_device_inputs'](userknn, *small)
    CASES['uknn_score_topk_device_inputs'](userknn, *big)
    after = CASES['uknn_score_topk_device_inputs'](userknn, *small)
    assert poison.compare(alone, after) == []

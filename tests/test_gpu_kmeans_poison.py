"""Poisoned scratch memory (tests/poison.py) for the k-means ops of arlib_amd/cluster.py: every output and workspace word is written before it is
read, so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file
applies the same introspection to the module these ops live in."""
import inspect

import numpy as np
import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def problem(N, k, d, seed):
    """Points, centroids and labels that leave cluster 1 empty (its row of C_new is a copy of C_prev, not scratch) and put half the rows into cluster 0 (past one chunk at the larger sizes)."""
    g = torch.Generator().manual_seed(seed)
    X, C = torch.randn(N, d, generator=g), torch.randn(k, d, generator=g)
    labels = torch.randint(2, k, (N,), generator=g)
    labels[torch.randperm(N, generator=g)[:N // 2]] = 0
    return X.to(DEV), C.to(DEV), labels.to(DEV)


def _kmeans(cl, X, C, labels, start):
    if start == 'given':
        return cl.kmeans(X, C.shape[0], n_iter=3, init=C)
    np.random.seed(X.shape[0])
    return cl.kmeans(X, C.shape[0], n_iter=3)


# ragged point tiles and more than one centroid stage / one wave and one ragged stage / the widest rows with a one-row second stage
SHAPES = [(1061, 200, 64), (130, 7, 16), (2049, 65, 128)]
CASES = {
    'kmeans_assign': lambda cl, X, C, labels: cl.kmeans_assign(X, C),
    'kmeans_update': lambda cl, X, C, labels: cl.kmeans_update(X, labels, C),
    'kmeans_update_int32': lambda cl, X, C, labels: cl.kmeans_update(X, labels.to(torch.int32), C, check_range=False),
    'kmeans': lambda cl, X, C, labels: _kmeans(cl, X, C, labels, 'given'),
    'kmeans_drawn_start': lambda cl, X, C, labels: _kmeans(cl, X, C, labels, 'drawn'),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import cluster
    found = introspected(inspect.getsource(cluster))
    assert {'kmeans_assign', 'kmeans_update'} <= found                      # the introspection sees the kernel wrappers' torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(cluster).items() if inspect.isfunction(f) and f.__module__ == cluster.__name__ and not n.startswith('_')}
    assert public - set(CASES) == {'kmeans_init_indices'}                   # host-only: numpy's draw, no device memory


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('N,k,d', SHAPES)
def test_op_is_independent_of_scratch_memory(name, N, k, d):
    from arlib_amd import cluster
    P = problem(N, k, d, seed=N)
    clean = CASES[name](cluster, *P)
    with poison.poisoned_allocations():
        dirty = CASES[name](cluster, *P)
    assert poison.compare(clean, dirty) == []                               # fixed-order reductions: the same bits
    assert not poison.has_nan(dirty)


def test_workspace_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import cluster
    big, small = problem(2049, 65, 128, seed=1), problem(700, 65, 128, seed=2)
    torch.cuda.empty_cache()
    alone = cluster.kmeans(small[0], 65, n_iter=3, init=small[1])
    cluster.kmeans(big[0], 65, n_iter=3, init=big[1])
    after = cluster.kmeans(small[0], 65, n_iter=3, init=small[1])
    assert poison.compare(alone, after) == []

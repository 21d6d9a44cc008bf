"""Poisoned scratch memory (tests/poison.py) for the k-means++ ops of arlib_amd/seeding.py: every output and workspace word is written before it is
read, so a run on NaN-filled allocations gives the bits of a clean run.  The sweep of test_gpu_poisoned_memory.py reads arlib_amd/ops.py; this file
applies the same introspection to the module these ops live in, as test_gpu_kmeans_poison.py does for arlib_amd/cluster.py."""
import inspect

import numpy as np
import pytest
import torch
import poison
from test_gpu_poisoned_memory import introspected

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def problem(N, k, d, seed):
    """Points, candidate ids (one repeated), a `closest` with zeros, and uniforms for the next draw."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, d, generator=g)
    T = 2 + int(np.log(k))
    ids = torch.randint(0, N, (T,), generator=g).to(torch.int32)
    ids[T - 1] = ids[0]
    closest = ((X - X[3]) ** 2).sum(1)
    u = torch.rand(T, generator=g, dtype=torch.float64)
    return X.to(DEV), k, ids.to(DEV), closest.to(DEV), u.to(DEV)


def _pick(sd, X, k, ids, closest, u, draw):
    mins, part = sd.kmeanspp_dist(X, ids, closest)
    return sd.kmeanspp_pick(mins, part, ids, u if draw else None)


def _seeded(X, run):
    np.random.seed(X.shape[0])
    return run()


# ragged spans and several of them / fewer rows than one sweep / the widest rows
SHAPES = [(1061, 200, 64), (130, 7, 16), (2049, 65, 128)]
CASES = {
    'kmeanspp_dist': lambda sd, cl, X, k, ids, closest, u: sd.kmeanspp_dist(X, ids, closest),
    'kmeanspp_dist_first_centre': lambda sd, cl, X, k, ids, closest, u: sd.kmeanspp_dist(X, ids[:1]),
    'kmeanspp_pick': lambda sd, cl, X, k, ids, closest, u: _pick(sd, X, k, ids, closest, u, True),
    'kmeanspp_pick_last_step': lambda sd, cl, X, k, ids, closest, u: _pick(sd, X, k, ids, closest, u, False),
    'kmeanspp': lambda sd, cl, X, k, ids, closest, u: _seeded(X, lambda: sd.kmeanspp(X, k)),
    'kmeanspp_traced': lambda sd, cl, X, k, ids, closest, u: _seeded(X, lambda: sd.kmeanspp(X, k, trace=True)),
    'kmeans_from_kmeanspp': lambda sd, cl, X, k, ids, closest, u: _seeded(X, lambda: cl.kmeans(X, k, n_iter=3, init='k-means++')),
}


def test_every_allocating_op_of_the_module_has_a_case():
    from arlib_amd import seeding
    found = introspected(inspect.getsource(seeding))
    assert {'kmeanspp_dist', 'kmeanspp_pick', 'kmeanspp'} <= found          # the introspection sees the wrappers' torch.empty
    assert sorted(found - set(CASES)) == []
    public = {n for n, f in vars(seeding).items() if inspect.isfunction(f) and f.__module__ == seeding.__name__ and not n.startswith('_')}
    assert public - set(CASES) == {'kmeanspp_draws'}                        # host-only: numpy's draws, no device memory


@pytest.mark.parametrize('name', sorted(CASES))
@pytest.mark.parametrize('N,k,d', SHAPES)
def test_op_is_independent_of_scratch_memory(name, N, k, d):
    from arlib_amd import cluster, seeding
    P = problem(N, k, d, seed=N)
    clean = CASES[name](seeding, cluster, *P)
    with poison.poisoned_allocations():
        dirty = CASES[name](seeding, cluster, *P)
    assert poison.compare(clean, dirty) == []                               # fixed-order reductions: the same bits
    assert not poison.has_nan(dirty)


def test_workspace_buffer_reused_between_shapes():
    """The caching allocator hands the second call the first call's blocks: results equal a fresh process's (a clean call after empty_cache)."""
    from arlib_amd import seeding
    big, small = problem(2049, 65, 128, seed=1), problem(700, 65, 128, seed=2)
    draws = (5, np.random.default_rng(3).random((64, 6)))
    torch.cuda.empty_cache()
    alone = seeding.kmeanspp(small[0], 65, draws=draws, trace=True)
    seeding.kmeanspp(big[0], 65, draws=draws, trace=True)
    after = seeding.kmeanspp(small[0], 65, draws=draws, trace=True)
    assert poison.compare(alone, after) == []

"""The device k-means++ start (arlib_amd/seeding.py, csrc/arl_kmeans.hip) without a GPU: the C entries reject bad arguments before any device work,
the draws are numpy's own in sklearn's order, the Python layer refuses what it cannot run before it touches a device or the generator, and NCL's
defaults stay where they were."""
import ctypes
import sys

import numpy as np
import pytest
import torch

E_NULL, E_DIM, E_RANGE, E_ARG = -1, -2, -3, -4
BIG = 2 ** 31 // 128 + 1


def _p(addr):
    return ctypes.c_void_p(addr)


def _each(call, good, cases):
    for i, value, want in cases:
        args = list(good)
        args[i] = value
        assert call(*args) == want, (i, value, want)


def test_c_entries_validate_before_any_device_work():
    from arlib_amd import _lib
    L = _lib.lib()
    a, odd16, odd8 = 4096, 4104, 4100                                       # never dereferenced: every call below returns before a launch
    # dist(X, N, d, cand_ids, n_cand, closest, mins, part, stream); closest may be NULL
    good = [_p(a), 8, 64, _p(a), 2, None, _p(a), _p(a), None]
    _each(L.arl_kmeanspp_dist_f32, good, [(i, None, E_NULL) for i in (0, 3, 6, 7)] + [(2, d, E_DIM) for d in (0, 8, 48, 65, 256)]
          + [(1, 0, E_ARG), (4, 0, E_ARG), (4, 17, E_ARG), (1, BIG, E_RANGE), (0, _p(odd16), E_ARG), (7, _p(odd8), E_ARG)])
    # pick(mins, part, N, n_cand, cand_ids, u, n_next, next_ids, winner, cand_pot, closest_out, stream); closest_out may be NULL, u / next_ids with n_next = 0
    good = [_p(a), _p(a), 8, 2, _p(a), _p(a), 2, _p(a), _p(a), _p(a), None, None]
    _each(L.arl_kmeanspp_pick_f64, good, [(i, None, E_NULL) for i in (0, 1, 4, 5, 7, 8, 9)]
          + [(2, 0, E_ARG), (3, 0, E_ARG), (3, 17, E_ARG), (6, -1, E_ARG), (6, 17, E_ARG), (2, BIG, E_RANGE), (1, _p(odd8), E_ARG), (5, _p(odd8), E_ARG),
             (9, _p(odd8), E_ARG)])
    # whole(X, N, d, k, n_trials, first, u, indices, closest, cand_ids, cand_pot, workspace, stream); the trace may be NULL, u with k = 1
    good = [_p(a), 100, 64, 5, 3, 7, _p(a), _p(a), _p(a), None, None, _p(a), None]
    _each(L.arl_kmeanspp_f32, good, [(i, None, E_NULL) for i in (0, 6, 7, 8, 11)] + [(2, d, E_DIM) for d in (0, 8, 48, 65, 256)]
          + [(1, 0, E_ARG), (3, 0, E_ARG), (3, 101, E_ARG), (4, 0, E_ARG), (4, 17, E_ARG), (5, -1, E_ARG), (5, 100, E_ARG), (1, BIG, E_RANGE),
             (0, _p(odd16), E_ARG), (11, _p(odd16), E_ARG), (6, _p(odd8), E_ARG), (10, _p(odd8), E_ARG)])
    # sizes: at most 1024 spans, every row in one; the workspace holds two sets of minima and the span partials
    assert L.arl_kmeanspp_spans(0) == 0 and L.arl_kmeanspp_spans(BIG) == 0
    for N in (1, 5, 130, 1061, 65801, 10 ** 6, BIG - 2):
        S, rows = L.arl_kmeanspp_spans(N), L.arl_kmeanspp_span_rows(N)
        assert 1 <= S <= 1024 and (S - 1) * rows < N <= S * rows
        for T in (1, 9, 16):
            assert L.arl_kmeanspp_workspace_bytes(N, T) >= 2 * 4 * T * N + 8 * T * S
    assert L.arl_kmeanspp_span_rows(0) == 0
    assert L.arl_kmeanspp_workspace_bytes(0, 3) == 0 and L.arl_kmeanspp_workspace_bytes(100, 0) == 0 and L.arl_kmeanspp_workspace_bytes(100, 17) == 0


@pytest.mark.parametrize('N,k,T', [(7, 1, 2), (5, 5, 3), (1412, 50, 5), (100000, 2000, 9)])
def test_draws_are_numpys_own_in_sklearns_order(N, k, T):
    from arlib_amd import seeding
    np.random.seed(11)
    want_first = np.random.choice(N, p=np.full(N, 1.0 / N))                 # _kmeans_plusplus: random_state.choice(n_samples, p=sample_weight / sample_weight.sum())
    want_u = np.stack([np.random.uniform(size=T) for _ in range(k - 1)]) if k > 1 else np.zeros((0, T))      # one call per step there
    after = np.random.random()
    np.random.seed(11)
    first, u = seeding.kmeanspp_draws(N, k)
    assert np.random.random() == after                                      # the generator is left where sklearn's own draws would leave it
    assert isinstance(first, int) and first == want_first and 0 <= first < N
    assert u.dtype == np.float64 and u.shape == (k - 1, T) and np.array_equal(u, want_u)


def test_refusals_come_before_the_library_and_the_generator(monkeypatch):
    from arlib_amd import cluster, seeding, _lib
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was reached'))
    for name in ('choice', 'uniform', 'random', 'random_sample', 'randint'):
        monkeypatch.setattr(np.random, name, lambda *a, **k: pytest.fail('the generator was advanced'))
    x = torch.zeros(10, 64)
    for run in (lambda t, k: seeding.kmeanspp(t, k), lambda t, k: cluster.kmeans(t, k, init='k-means++')):
        with pytest.raises(ValueError, match='must be on the GPU'):
            run(x, 3)                                                       # a host tensor: no silent fallback
        with pytest.raises(ValueError, match='2-d torch.Tensor'):
            run(x.numpy(), 3)
        for dtype in (torch.float64, torch.float16, torch.int32):
            with pytest.raises(ValueError, match='must be float32'):
                run(torch.zeros(10, 64, dtype=dtype), 3)
        for width in (8, 24, 65, 256):
            with pytest.raises(ValueError, match='width %d outside' % width):
                run(torch.zeros(10, width), 3)
        with pytest.raises(ValueError, match='n_samples=10 should be >= n_clusters=11'):
            run(x, 11)
        for k in (0, -1):
            with pytest.raises(ValueError, match='at least one cluster'):
                run(x, k)
    for init in ('random', 'kmeans++', 'k-means||', ''):
        with pytest.raises(ValueError, match='init must be'):
            cluster.kmeans(x, 3, init=init)
    # the step wrappers too
    with pytest.raises(ValueError, match='must be on the GPU'):
        seeding.kmeanspp_dist(x, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError, match='on the GPU'):
        seeding.kmeanspp_pick(torch.zeros(2, 10), torch.zeros(2, 1, dtype=torch.float64), torch.zeros(2, dtype=torch.int32))


def test_ncl_start_defaults_to_random_rows_and_the_default_route_imports_no_device_module(monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from test_host_api import make_data
    import arlib_amd
    from arlib_amd.recommender.NCL import NCL
    assert NCL.kmeans_init == 'random' and NCL.kmeans == 'sklearn'
    args = dict(dataset='ml-100k', model_name='NCL', maxEpoch=30, batch_size=2048, emb_size=16, n_layers=2, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    data = make_data()
    with contextlib.redirect_stdout(io.StringIO()):
        rec, pp = NCL(SimpleNamespace(**args), data), NCL(SimpleNamespace(ncl_kmeans='device', ncl_kmeans_init='k-means++', **args), data)
        for bad in ('kmeans++', 'k-means||', None):
            with pytest.raises(ValueError, match='kmeans_init'):
                NCL(SimpleNamespace(ncl_kmeans_init=bad, **args), data)
    assert (rec.kmeans, rec.kmeans_init) == ('sklearn', 'random') and (pp.kmeans, pp.kmeans_init) == ('device', 'k-means++') and NCL.kmeans_init == 'random'
    # the default route is the reference's host call: an import of either device module would fail here
    with monkeypatch.context() as m:
        for name in ('cluster', 'seeding'):
            m.setitem(sys.modules, 'arlib_amd.' + name, None)
            m.delattr(arlib_amd, name, raising=False)
        rec.k = 20
        np.random.seed(515)
        rec.e_step()
    assert rec.user_centroids.shape == (20, 16) and rec.item_2cluster.shape == (data.item_num,)
    # and the opt-in route has no host fallback: without a GPU it raises before a draw
    pp.k = 20
    state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError, match='must be on the GPU'):
        pp.e_step()
    assert np.array_equal(np.random.get_state()[1], state)

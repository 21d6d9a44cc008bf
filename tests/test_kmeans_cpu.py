"""Device k-means (arlib_amd/cluster.py, csrc/arl_kmeans.hip) without a GPU: the C entries reject bad arguments before any device work, the loop
rejects what it cannot run before it touches a device, the start rows are numpy's own draw, and NCL's default back end stays sklearn."""
import ctypes

import numpy as np
import pytest
import torch

E_NULL, E_DIM, E_RANGE, E_ARG = -1, -2, -3, -4


def _p(addr):
    return ctypes.c_void_p(addr)


def test_c_entries_validate_before_any_device_work():
    from arlib_amd import _lib
    L = _lib.lib()
    a, odd = 4096, 4100                                                     # never dereferenced: every call below returns before a launch
    # assign(X, N, C, k, d, bias, labels, score, stream)
    assert L.arl_kmeans_assign_f32(None, 8, _p(a), 2, 64, _p(a), _p(a), _p(a), None) == E_NULL
    assert L.arl_kmeans_assign_f32(_p(a), 8, None, 2, 64, _p(a), _p(a), _p(a), None) == E_NULL
    assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 2, 64, None, _p(a), _p(a), None) == E_NULL
    assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 2, 64, _p(a), None, _p(a), None) == E_NULL
    assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 2, 64, _p(a), _p(a), None, None) == E_NULL
    for d in (0, 8, 48, 65, 256):
        assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 2, d, _p(a), _p(a), _p(a), None) == E_DIM
    assert L.arl_kmeans_assign_f32(_p(a), 0, _p(a), 2, 64, _p(a), _p(a), _p(a), None) == E_ARG
    assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 0, 64, _p(a), _p(a), _p(a), None) == E_ARG
    assert L.arl_kmeans_assign_f32(_p(a), 2 ** 31 // 128 + 1, _p(a), 2, 64, _p(a), _p(a), _p(a), None) == E_RANGE
    assert L.arl_kmeans_assign_f32(_p(a), 8, _p(a), 2 ** 31 // 128 + 1, 64, _p(a), _p(a), _p(a), None) == E_RANGE
    assert L.arl_kmeans_assign_f32(_p(odd), 8, _p(a), 2, 64, _p(a), _p(a), _p(a), None) == E_ARG
    # update(X, N, d, order, seg_ptr, chunk_ptr, k, C_prev, C_new, workspace, stream)
    good = [_p(a), 8, 64, _p(a), _p(a), _p(a), 2, _p(a), _p(2 * a), _p(a), None]
    for i in (0, 3, 4, 5, 7, 8, 9):
        args = list(good); args[i] = None
        assert L.arl_kmeans_update_f32(*args) == E_NULL
    args = list(good); args[2] = 24
    assert L.arl_kmeans_update_f32(*args) == E_DIM
    args = list(good); args[1] = 0
    assert L.arl_kmeans_update_f32(*args) == E_ARG
    args = list(good); args[6] = 0
    assert L.arl_kmeans_update_f32(*args) == E_ARG
    args = list(good); args[8] = args[7]                                    # C_new aliases C_prev
    assert L.arl_kmeans_update_f32(*args) == E_ARG
    args = list(good); args[1] = 2 ** 31 // 128 + 1
    assert L.arl_kmeans_update_f32(*args) == E_RANGE
    args = list(good); args[9] = _p(odd)
    assert L.arl_kmeans_update_f32(*args) == E_ARG
    # sum(v, n, squared, out, workspace, stream)
    assert L.arl_kmeans_sum_f64(None, 8, 0, _p(a), _p(a), None) == E_NULL
    assert L.arl_kmeans_sum_f64(_p(a), 8, 0, None, _p(a), None) == E_NULL
    assert L.arl_kmeans_sum_f64(_p(a), 8, 0, _p(a), None, None) == E_NULL
    assert L.arl_kmeans_sum_f64(_p(a), 0, 0, _p(a), _p(a), None) == E_ARG
    assert L.arl_kmeans_sum_f64(_p(a), 8, 0, _p(odd), _p(a), None) == E_ARG
    # sizes: room for every chunk (sum_c ceil(n_c / chunk) <= N / chunk + k) and for the spans of the double sums
    chunk = L.arl_kmeans_chunk_rows()
    assert chunk >= 1
    assert L.arl_kmeans_update_workspace_bytes(20011, 3, 64) == 4 * 64 * (20011 // chunk + 3)
    assert L.arl_kmeans_update_workspace_bytes(20011, 3, 24) == 0 and L.arl_kmeans_update_workspace_bytes(0, 3, 64) == 0
    assert L.arl_kmeans_sum_workspace_bytes() >= 8 and L.arl_kmeans_sum_workspace_bytes() % 8 == 0


def test_kmeans_rejects_what_it_cannot_run(monkeypatch):
    from arlib_amd import cluster, _lib
    monkeypatch.setattr(_lib, 'lib', lambda: pytest.fail('the library was reached'))
    assert cluster.KMEANS_WIDTHS == (16, 32, 64, 128)
    x = torch.zeros(10, 64)
    with pytest.raises(ValueError, match='must be on the GPU'):
        cluster.kmeans(x, 3)                                                # a host tensor: no silent fallback
    with pytest.raises(ValueError, match='2-d torch.Tensor'):
        cluster.kmeans(x.numpy(), 3)
    with pytest.raises(ValueError, match='2-d torch.Tensor'):
        cluster.kmeans(torch.zeros(64), 3)
    # each refusal for the reason it names (width, then dtype, then device: a host tensor of a bad width or dtype says so)
    for dtype in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(ValueError, match='must be float32'):
            cluster.kmeans(torch.zeros(10, 64, dtype=dtype), 3)
    for width in (8, 24, 65, 256):
        with pytest.raises(ValueError, match='width %d outside' % width):
            cluster.kmeans(torch.zeros(10, width), 3)
    # the sizes: sklearn raises for n_samples < n_clusters too
    monkeypatch.setattr(np.random, 'choice', lambda *a, **k: pytest.fail('the generator was advanced'))
    with pytest.raises(ValueError, match='n_samples=10 should be >= n_clusters=11'):
        cluster.kmeans(x, 11)
    for k in (0, -1):
        with pytest.raises(ValueError, match='at least one cluster'):
            cluster.kmeans(x, k)
    with pytest.raises(ValueError, match='n_iter'):
        cluster.kmeans(x, 3, n_iter=-1)
    for fn in (cluster.kmeans_assign, lambda a, b: cluster.kmeans_update(a, torch.zeros(10, dtype=torch.int64), b)):
        with pytest.raises(ValueError):
            fn(x, torch.zeros(3, 64))


@pytest.mark.parametrize('N,k', [(1412, 50), (100000, 2000), (5, 5), (7, 1)])
def test_init_indices_are_numpys_own_draw(N, k):
    from arlib_amd import cluster
    np.random.seed(7)
    want = np.random.choice(N, k, replace=False)
    after = np.random.random()
    np.random.seed(7)
    got = cluster.kmeans_init_indices(N, k)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.random.random() == after                                      # the generator is left where sklearn's own draw would leave it
    assert len(set(got.tolist())) == k and 0 <= got.min() and got.max() < N


def test_ncl_default_backend_is_sklearn(monkeypatch):
    import contextlib
    import io
    from types import SimpleNamespace
    from test_host_api import make_data
    from arlib_amd import cluster
    from arlib_amd.recommender.NCL import NCL
    assert NCL.kmeans == 'sklearn'
    args = dict(dataset='ml-100k', model_name='NCL', maxEpoch=30, batch_size=2048, emb_size=16, n_layers=2, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    data = make_data()
    with contextlib.redirect_stdout(io.StringIO()):
        rec, dev = NCL(SimpleNamespace(**args), data), NCL(SimpleNamespace(ncl_kmeans='device', **args), data)
        with pytest.raises(ValueError):
            NCL(SimpleNamespace(ncl_kmeans='faiss', **args), data)
    assert rec.kmeans == 'sklearn' and dev.kmeans == 'device' and NCL.kmeans == 'sklearn'
    # the default route is the reference's host call and never reaches the device module (host tensors here: sklearn does not need a GPU)
    with monkeypatch.context() as m:
        m.setattr(cluster, 'kmeans', lambda *a, **k: pytest.fail('cluster.kmeans was called'))
        rec.k = 20
        np.random.seed(515)
        rec.e_step()
    assert rec.user_centroids.shape == (20, 16) and rec.user_centroids.dtype == torch.float32 and rec.item_2cluster.dtype == torch.int64
    assert rec.item_2cluster.shape == (data.item_num,) and int(rec.item_2cluster.max()) < 20
    # and the opt-in route has no host fallback: without a GPU it raises instead of clustering somewhere else
    dev.k = 20
    with pytest.raises(ValueError):
        dev.e_step()

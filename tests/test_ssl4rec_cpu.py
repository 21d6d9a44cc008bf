"""SSL4Rec without a GPU: the initial parameters under seedSet(2018) equal the reference's bit for bit (g29), the parameter order and names,
the deterministic dropout rule of tests/golden/gen_golden_ssl4rec.py, and a numpy restatement of the in-kernel mask hash
(include/arlib_amd.h, arl_ssl_dropout_nce_f32).  The restatement and the rule are what tests/test_gpu_ssl4rec.py feeds the kernel with."""
import hashlib
import numpy as np
import pytest
import torch
from types import SimpleNamespace
from conftest import golden
from test_host_api import make_data

DROP = 0.2
_M64 = (1 << 64) - 1


def rule_mask(t, c, n, d):
    """gen_golden_ssl4rec.py's dropout rule: call c (0/1: user views 1/2, 2/3: item views 1/2) of step t keeps (i, k) iff rng.random >= 0.2."""
    return np.random.default_rng([2018, t, c]).random((n, d)) >= DROP


def rule_view_masks(t, n, d):
    """The rule's masks of step t as the kernel's [2 sides][2 views][n][d] (side 0 = users, 1 = positives)."""
    return np.stack([rule_mask(t, c, n, d) for c in range(4)]).reshape(2, 2, n, d)


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def hash_view_masks(seed, stream, n, d, p=DROP):
    """The in-kernel masks: kept iff (splitmix64(key ^ (((sv << 32) + i) * d + k)) >> 40) * 2^-24 >= p, key = splitmix64(seed ^ stream * golden)."""
    with np.errstate(over='ignore'):
        key = _splitmix64(np.array([(seed ^ ((stream * 0x9E3779B97F4A7C15) & _M64)) & _M64], np.uint64))[0]
        sv = np.arange(4, dtype=np.uint64)[:, None, None]
        i = np.arange(n, dtype=np.uint64)[None, :, None]
        k = np.arange(d, dtype=np.uint64)[None, None, :]
        c = ((sv << np.uint64(32)) + i) * np.uint64(d) + k
        u = (_splitmix64(key ^ c) >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (u >= np.float32(p)).reshape(2, 2, n, d)


def rec_args(**kw):
    a = dict(dataset='ml-100k', model_name='SSL4Rec', maxEpoch=30, batch_size=2048, emb_size=64, n_layers=3, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


def test_initial_parameters_order_and_names_match_reference():
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.SSL4Rec import SSL4Rec
    g = golden('g29_ssl4rec.npz')
    seedSet(2018)
    rec = SSL4Rec(rec_args(), make_data())
    names = [n for n, _ in rec.model.named_parameters()]
    assert names == [str(x) for x in g['param_names']]
    assert names[:8] == ['user_tower.0.weight', 'user_tower.0.bias', 'user_tower.2.weight', 'user_tower.2.bias',
                         'item_tower.0.weight', 'item_tower.0.bias', 'item_tower.2.weight', 'item_tower.2.bias']
    assert names[8:] == ['embedding_dict.item_emb', 'embedding_dict.user_emb']
    for n, p in rec.model.named_parameters():
        v = p.detach().cpu().numpy()
        assert hashlib.sha256(np.ascontiguousarray(v, np.float32).tobytes()).hexdigest() == str(g['init_sha__' + n]), n
        assert np.array_equal(v.reshape(v.shape[0], -1)[0], g['init_probe__' + n]), n
    # the towers are registered but never trained, and their digests after the reference's 25 Adam steps are the initial ones
    for n in names[:8]:
        assert str(g['tower_sha__' + n]) == str(g['init_sha__' + n])


def test_rule_masks_match_fixture_digest():
    g = golden('g29_ssl4rec.npz')
    h = hashlib.sha256()
    for t, n in enumerate(g['batch_sizes']):
        for c in range(4):
            h.update(np.ascontiguousarray(rule_mask(t, c, int(n), 64), dtype=np.bool_).tobytes())
    assert h.hexdigest() == str(g['mask_sha'])
    m = rule_view_masks(3, int(g['batch_sizes'][3]), 64)
    assert np.array_equal(m[1, 0], rule_mask(3, 2, int(g['batch_sizes'][3]), 64))


@pytest.mark.parametrize('seed,stream', [(0, 0), (12345, 7), (2 ** 62 - 1, 2 ** 40)])
def test_mask_hash_keep_fraction_within_binomial_bounds(seed, stream):
    n, d = 2048, 64
    m = hash_view_masks(seed, stream, n, d)
    N = m.size
    sd = np.sqrt(N * DROP * (1 - DROP))
    assert abs(m.sum() - N * (1 - DROP)) < 6 * sd
    # each (side, view) is its own draw, and the next stream differs
    assert not np.array_equal(m[0, 0], m[0, 1]) and not np.array_equal(m[0, 0], m[1, 0])
    assert not np.array_equal(m, hash_view_masks(seed, stream + 1, n, d))
    # p = 0 keeps everything
    assert hash_view_masks(seed, stream, 4, 16, p=0.0).all()

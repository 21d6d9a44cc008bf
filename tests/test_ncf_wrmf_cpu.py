"""NCF and WRMF without a GPU: initial parameters under seedSet(2018) equal the reference's bit for bit (g27 / g28), parameter order and names,
the reference's errors for what a graph-less model cannot do, and wrmf_loss on CPU tensors.  Also the helpers the GPU tests read the compact
fixtures with (tests/golden/gen_golden_models.py: sampled rows of large arrays, digests of what a test rebuilds exactly)."""
import hashlib
import random
import numpy as np
import pytest
import torch
from types import SimpleNamespace
from conftest import golden
from test_host_api import make_data


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr, dtype=np.float32).tobytes()).hexdigest()


def pick(arr, g, key):
    """The rows of `arr` the fixture stored for `key` (all of them when the array was stored whole), as numpy."""
    arr = arr.detach().cpu().numpy() if isinstance(arr, torch.Tensor) else np.asarray(arr)
    return arr[g[key + '__rows']] if key + '__rows' in g.files else arr


def golden_batches(g):
    """The fixture's training batches, rebuilt by the drop-in sampler (bit-exact with the reference's after random.seed(2018) on a fresh
    DataLoader) and checked against the stored digest."""
    from arlib_amd.util.sampler import next_batch_pairwise
    n = len(g['batch_sizes'])
    data = make_data()
    random.seed(2018)
    out = []
    while len(out) < n:
        for b in next_batch_pairwise(data, 2048):
            out.append(tuple(np.asarray(x, np.int32) for x in b))
            if len(out) == n:
                break
    h = hashlib.sha256()
    for b in out:
        for x in b:
            h.update(x.tobytes())
    assert h.hexdigest() == str(g['batches_sha'])
    return out


def rec_args(**kw):
    a = dict(dataset='ml-100k', maxEpoch=30, batch_size=2048, emb_size=64, n_layers=3, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


def _build(name):
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.NCF import NCF
    from arlib_amd.recommender.WRMF import WRMF
    cls, g = (NCF, golden('g27_ncf.npz')) if name == 'ncf' else (WRMF, golden('g28_wrmf.npz'))
    seedSet(2018)
    return cls(rec_args(model_name=cls.__name__), make_data()), g


@pytest.mark.parametrize('name', ['ncf', 'wrmf'])
def test_initial_parameters_match_reference_bit_for_bit(name):
    rec, g = _build(name)
    names = [n for n, _ in rec.model.named_parameters()]
    assert names == list(g['param_names'])                                     # same names, same order (parameters() feeds Adam)
    for n, p in rec.model.named_parameters():
        v = p.detach().cpu().numpy()
        assert np.array_equal(v.reshape(v.shape[0], -1)[0], g['init_probe__' + n]) and sha(v) == str(g['init_sha__' + n]), n


def test_ncf_parameter_order_and_modules():
    rec, _ = _build('ncf')
    m = rec.model
    assert isinstance(m._fc_layers, torch.nn.ModuleList) and [tuple(l.weight.shape) for l in m._fc_layers] == [(320, 64), (128, 320), (64, 128)]
    assert [n for n, _ in m.named_parameters()] == ['_fc_layers.0.weight', '_fc_layers.0.bias', '_fc_layers.1.weight', '_fc_layers.1.bias',
                                                    '_fc_layers.2.weight', '_fc_layers.2.bias', 'embedding_dict.item_mf_emb',
                                                    'embedding_dict.item_mlp_emb', 'embedding_dict.user_mf_emb', 'embedding_dict.user_mlp_emb']
    assert len(list(m.parameters())) == 10


def test_ncf_requires_adjgrad_raises_reference_error_before_work():
    rec, _ = _build('ncf')
    before = [p.detach().clone() for p in rec.model.parameters()]
    with pytest.raises(AttributeError, match="'NCFEncoder' object has no attribute 'sparse_norm_adj'"):
        rec.train(requires_adjgrad=True, Epoch=1)
    assert all(torch.equal(a, b) for a, b in zip(before, rec.model.parameters()))
    assert not hasattr(rec, 'Matgrad') and not hasattr(rec, 'bestPerformance') or rec.bestPerformance == []


@pytest.mark.parametrize('name', ['ncf', 'wrmf'])
def test_init_uiadj_raises_reference_error(name):
    rec, _ = _build(name)
    with pytest.raises(Exception, match='This model hava no graph'):
        rec.model._init_uiAdj(None)


def test_wrmf_loss_matches_golden_step0_on_cpu():
    """wrmf_loss + l2_reg_loss of the golden's first batch on the initial CPU tables reproduce the reference's first loss."""
    from arlib_amd.util.loss import wrmf_loss
    rec, g = _build('wrmf')
    u0, i0 = (rec.model.embedding_dict[k].detach() for k in ('user_emb', 'item_emb'))
    assert sha(u0.numpy()) == str(g['init_sha__embedding_dict.user_emb'])
    bu, bp, bn = (torch.from_numpy(x).long() for x in golden_batches(g)[0])
    ue, pe, ne = u0[bu], i0[bp], i0[bn]
    loss = wrmf_loss(ue, pe, ne) + 1e-4 * (torch.norm(ue, p=2) + torch.norm(pe, p=2))
    assert abs(float(loss) - float(g['losses'][0])) <= 1e-5 * abs(float(g['losses'][0]))
    # pos_weight is honoured and the term is a sum, not a mean
    one = wrmf_loss(ue[:1], pe[:1], ne[:1], pos_weight=3)
    ps, ns = float((ue[0] * pe[0]).sum()), float((ue[0] * ne[0]).sum())
    assert abs(float(one) - (3 * (ps - 1) ** 2 + ns ** 2)) < 1e-5

"""DirectAU(args, data) on the MI355X against the reference's own pieces run as DirectAU's loop (g34_directau.npz: ml-100k, d 64, L 2, seed 2018):
the forward, the step-0 gradients, 25 Adam steps, the train() surface with requires_embgrad, copies, and the sampler's `random` stream.  The bars
are those of tests/test_gpu_ssl4rec.py's golden tests."""
import contextlib
import copy
import io
import pickle
import random
from types import SimpleNamespace
import numpy as np
import pytest
import torch
from conftest import golden, close, rel_err
from test_host_api import make_data
from test_ncf_wrmf_cpu import pick, golden_batches

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')


def rec_args(**kw):
    a = dict(dataset='ml-100k', model_name='DirectAU', maxEpoch=30, batch_size=2048, emb_size=64, n_layers=2, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


def _fresh(cls=None, **kw):
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender import DirectAU
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = (cls or DirectAU)(rec_args(**kw), make_data())
    return rec


def _terms(rec, u, p):
    from arlib_amd.util.loss import alignment_loss, uniformity_loss
    return alignment_loss(u, p), rec.gamma * (uniformity_loss(u) + uniformity_loss(p)) / 2


def test_golden_forward_step0_gradients_and_25_adam_steps():
    from arlib_amd.util.loss import l2_reg_loss
    g = golden('g34_directau.npz')
    rec = _fresh()
    model = rec.model.cuda()
    assert rec.gamma == 2.0 and rec.l2_scale == 1.0 / 2048 and rec._fusable(torch.optim.Adam(model.parameters(), lr=0.005)) is None
    with torch.no_grad():
        u, i = model()
    assert close(pick(u, g, 'fwd_user'), g['fwd_user']) and close(pick(i, g, 'fwd_item'), g['fwd_item'])
    batches = golden_batches(g)
    reg = rec.args.reg * rec.l2_scale
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    al, un = [], []
    for step, batch in enumerate(batches):
        bu, bp, bn = (torch.from_numpy(x).long().to(DEV) for x in batch)
        ue, ie = model()
        loss = rec._batch_loss(ue[bu], ie[bp], ie[bn], reg)
        with torch.no_grad():
            a, b = _terms(rec, ue[bu], ie[bp])
            assert torch.equal(loss.detach(), a + b + l2_reg_loss(reg, ue[bu], ie[bp]))          # the class's loss is the three terms, negatives unread
        al.append(float(a)); un.append(float(b))
        opt.zero_grad()
        loss.backward()
        if step == 0:
            for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
                assert close(pick(dict(model.named_parameters())[n].grad, g, 'grad0__' + n), g['grad0__' + n]), n
        opt.step()
    assert np.allclose(al[:3], g['align_losses'][:3], rtol=1e-5, atol=0) and np.allclose(un[:3], g['unif_losses'][:3], rtol=1e-5, atol=0)
    assert np.allclose(al, g['align_losses'], rtol=1e-3, atol=0) and np.allclose(un, g['unif_losses'], rtol=1e-3, atol=0)
    params = dict(model.named_parameters())
    for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
        assert close(pick(params[n], g, 'final__' + n), g['final__' + n], tol=1e-2), n


def test_train_api_embgrad_and_copies_match_reference_run():
    g = golden('g34_directau.npz')
    rec = _fresh()
    with contextlib.redirect_stdout(io.StringIO()):
        ue, ie, ug, ig = rec.train(Epoch=2, evalNum=1, requires_embgrad=True)
        _, measure = rec.test()
    assert random.random() == float(g['api_next_random'][0])
    assert not rec.last_train_stats['fused']
    assert rel_err(pick(ue, g, 'api_user_emb'), g['api_user_emb']) < 1e-2 and rel_err(pick(ie, g, 'api_item_emb'), g['api_item_emb']) < 1e-2
    assert rel_err(pick(ug, g, 'api_usergrad'), g['api_usergrad']) < 1e-2 and rel_err(pick(ig, g, 'api_itemgrad'), g['api_itemgrad']) < 1e-2
    assert rec.bestPerformance[0] == int(g['api_best_epoch'][0])
    got = np.array([float(m.strip().split(':')[1]) for m in measure[1:]])
    assert np.allclose(got, g['api_measure'], rtol=0, atol=2e-3)
    for r in (copy.deepcopy(rec), pickle.loads(pickle.dumps(rec))):
        assert r.gamma == rec.gamma and r.l2_scale == rec.l2_scale
        assert rel_err(r.model()[0].detach().cpu().numpy(), rec.model()[0].detach().cpu().numpy()) < 1e-6


def test_gamma_override_adjgrad_surface_and_lightgcn_random_stream():
    from arlib_amd.recommender.LightGCN import LightGCN
    rec = _fresh(directau_gamma=0.5)
    assert rec.gamma == 0.5 and type(rec).gamma == 2.0
    random.seed(77)
    with contextlib.redirect_stdout(io.StringIO()):
        block = rec.train(Epoch=1, evalNum=1, requires_adjgrad=True)
    state = random.getstate()
    assert tuple(block.shape) == (rec.data.user_num, rec.data.item_num) and bool(torch.isfinite(block).all()) and bool(block.any())
    lgn = _fresh(LightGCN)
    random.seed(77)
    with contextlib.redirect_stdout(io.StringIO()):
        lgn.train(Epoch=1, evalNum=1)
    assert random.getstate() == state                                     # the negatives are drawn although the loss does not read them

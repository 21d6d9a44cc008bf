"""WRMF on the MI355X: the fused WRMF + L2 kernel (ops.wrmf_l2_fwd_bwd) against float64, and WRMF(args, data) against the reference's own run
(tests/golden/g28_wrmf.npz, gen_golden_models.py)."""
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
    a = dict(dataset='ml-100k', model_name='WRMF', maxEpoch=30, batch_size=2048, emb_size=64, n_layers=3, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize('B', [1, 37, 2049])
@pytest.mark.parametrize('d', [16, 64, 100])
def test_wrmf_kernel_against_float64_with_duplicates(B, d):
    from arlib_amd import ops
    gen = torch.Generator().manual_seed(B * 7 + d)
    U, I, reg = 300, 200, 1e-2
    E = torch.randn(U + I, d, generator=gen, dtype=torch.float64) * 0.2
    u, p, n = torch.randint(0, U, (B,), generator=gen), torch.randint(0, I, (B,), generator=gen), torch.randint(0, I, (B,), generator=gen)
    u[: B // 2] = u[0]; p[: B // 3] = n[0]                                  # duplicate users; an item both positive and negative
    Er = E.clone().requires_grad_(True)
    ue, pe, ne = Er[u], Er[U + p], Er[U + n]
    ps, ns = (ue * pe).sum(1), (ue * ne).sum(1)
    ref = (20 * (ps - 1) ** 2 + ns ** 2).sum() + reg * (torch.norm(ue) + torch.norm(pe))
    ref.backward()
    Ed = E.float().to(DEV)
    G = torch.zeros_like(Ed)
    i32 = lambda t: t.to(torch.int32).to(DEV)
    out = ops.wrmf_l2_fwd_bwd(Ed, U, i32(u), i32(p), i32(n), reg, 20.0, G)
    ref = float(ref.detach())
    assert abs(float(out[0] + out[1]) - ref) <= 1e-5 * abs(ref)
    assert close(G.cpu().numpy(), Er.grad.numpy())
    G2 = torch.zeros_like(Ed)
    ops.wrmf_l2_fwd_bwd(Ed, U, i32(u), i32(p), i32(n), reg, 20.0, G2)
    assert torch.equal(G, G2)                                                 # bit-identical from run to run


def _fresh():
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.WRMF import WRMF
    seedSet(2018)
    return WRMF(rec_args(), make_data())


def test_wrmf_loss_functions_against_reference_expression():
    from arlib_amd.util.loss import wrmf_loss, wrmf_l2_loss
    gen = torch.Generator().manual_seed(5)
    u, p, n = (torch.randn(300, 64, generator=gen) * 0.3 for _ in range(3))
    ref = wrmf_loss(u, p, n)                                                  # CPU: the reference's expression
    ud, pd, nd = (t.to(DEV).requires_grad_(True) for t in (u, p, n))
    got = wrmf_loss(ud, pd, nd)
    assert abs(float(got.detach()) - float(ref)) <= 1e-5 * abs(float(ref))
    got2 = wrmf_l2_loss(ud, pd, nd, 1e-3)
    assert abs(float(got2.detach()) - float(ref + 1e-3 * (torch.norm(u) + torch.norm(p)))) <= 1e-5 * abs(float(ref))


def test_wrmf_golden_forward_step0_gradients_and_25_adam_steps():
    """Forward, step-0 gradients and the 25 losses at 1e-4.  The tables after 25 Adam steps at 5e-4 (measured 3.3e-4 max-norm on the item table):
    a negative item's gradient is 2 <u,n> u, and where <u,n> is near 0 its fp32 rounding is a large fraction of it, which Adam's g / sqrt(v)
    turns into steps of up to lr whatever the gradient's size (the NCL test above states the same for its tables)."""
    g = golden('g28_wrmf.npz')
    rec = _fresh()
    assert rec._fusable(torch.optim.Adam(rec.model.parameters(), lr=0.005)) is None      # never the BPR engine step
    model = rec.model.cuda()
    u, i = model()
    assert u is model.embedding_dict['user_emb']                               # GMF's aliasing quirk kept
    assert close(pick(u, g, 'fwd_user'), g['fwd_user']) and close(pick(i, g, 'fwd_item'), g['fwd_item'])
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    U = rec.data.user_num
    losses = []
    for s, batch in enumerate(golden_batches(g)):
        bu, bp, bn = (torch.from_numpy(x).to(DEV) for x in batch)
        B = bu.numel()
        out = model.forward_rows(torch.cat([bu, bp + U, bn + U]).to(torch.int32))
        loss = rec._batch_loss(out[:B], out[B:2 * B], out[2 * B:], 1e-4)
        opt.zero_grad()
        loss.backward()
        if s == 0:
            for n, p in model.named_parameters():
                assert close(pick(p.grad, g, 'grad0__' + n), g['grad0__' + n]), n
        opt.step()
        losses.append(float(loss.detach()))
    assert np.allclose(losses, g['losses'], rtol=1e-4, atol=0)
    params = dict(model.named_parameters())
    for n, p in params.items():
        assert close(pick(p, g, 'final__' + n), g['final__' + n], tol=5e-4, row_tol=1e-3), n
    st = opt.state[params[str(g['adam_state_param'])]]
    assert close(pick(st['exp_avg'], g, 'm_state'), g['m_state'], tol=5e-4, row_tol=1e-3)
    assert close(pick(st['exp_avg_sq'], g, 'v_state'), g['v_state'], tol=5e-4, row_tol=1e-3)


@pytest.mark.parametrize('embgrad', [True, False])
def test_wrmf_train_api_matches_reference_run_and_survives_copies(embgrad):
    """With the default optimizer (torch.optim.Adam over the two tables: what would select the BPR-only fused step) and with requires_embgrad.
    Tables after the 44 steps at 5e-4 / row-wise 1e-3 (measured 2.0e-4 / 4.2e-4; why they drift past 1e-4: see the test above)."""
    g = golden('g28_wrmf.npz')
    rec = _fresh()
    with contextlib.redirect_stdout(io.StringIO()):
        ret = rec.train(Epoch=2, evalNum=1, requires_embgrad=embgrad)
        _, measure = rec.test()
    assert random.random() == float(g['api_next_random'][0])
    assert not rec.last_train_stats['fused']
    if embgrad:
        ue, ie, ug, ig = ret
        assert close(pick(ug, g, 'api_usergrad'), g['api_usergrad'], tol=5e-4, row_tol=1e-3) and close(pick(ig, g, 'api_itemgrad'), g['api_itemgrad'], tol=5e-4, row_tol=1e-3)
    else:
        assert ret is None
        ue, ie = rec.user_emb, rec.item_emb
    assert close(pick(ue, g, 'api_user_emb'), g['api_user_emb'], tol=5e-4, row_tol=1e-3) and close(pick(ie, g, 'api_item_emb'), g['api_item_emb'], tol=5e-4, row_tol=1e-3)
    assert rec.bestPerformance[0] == int(g['api_best_epoch'][0])
    got = np.array([float(m.strip().split(':')[1]) for m in measure[1:]])
    assert np.allclose(got, g['api_measure'], rtol=0, atol=2e-3)
    ref_u = rec.model()[0].detach().cpu().numpy()
    for r in (copy.deepcopy(rec), pickle.loads(pickle.dumps(rec))):
        assert rel_err(r.model()[0].detach().cpu().numpy(), ref_u) < 1e-6
    with pytest.raises(Exception, match='This model hava no graph'):
        rec.model._init_uiAdj(None)

"""SSL4Rec on the MI355X: the dropout-view InfoNCE kernel (ops.ssl_dropout_nce) against float64 torch, the fused step
(engine.step_ssl4rec) against a float64 SSL4Rec step written here and against the class's autograd route, and SSL4Rec(args, data) against
the reference's own run with the deterministic dropout rule of tests/golden/gen_golden_ssl4rec.py (g29_ssl4rec.npz)."""
import contextlib
import copy
import ctypes as C
import io
import pickle
import random
from types import SimpleNamespace
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from conftest import golden, close, rel_err
from test_host_api import make_data
from test_ncf_wrmf_cpu import pick, golden_batches
from test_ssl4rec_cpu import rule_view_masks, hash_view_masks

pytestmark = pytest.mark.gpu
DEV = 'cuda'
WIDTHS = (16, 32, 64, 128)


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')


def rec_args(**kw):
    a = dict(dataset='ml-100k', model_name='SSL4Rec', maxEpoch=30, batch_size=2048, emb_size=64, n_layers=3, reg=1e-4, lRate=0.005, seed=2018, topK='50')
    a.update(kw)
    return SimpleNamespace(**a)


def ref_term(Xu, Xp, masks, p=0.2, tau=0.2):
    """float64: (loss_u, loss_p) and their gradients w.r.t. Xu, Xp (util/loss.py:42-49 on dropout views)."""
    Xu = Xu.double().detach().requires_grad_(True)
    Xp = Xp.double().detach().requires_grad_(True)
    m = masks.double()
    s = 1.0 / (1.0 - p)

    def nce(v1, v2):
        a, b = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
        lg = a @ b.T / tau
        return (torch.logsumexp(lg, 1) - lg.diagonal()).mean()
    lu = nce(Xu * m[0, 0] * s, Xu * m[0, 1] * s)
    lp = nce(Xp * m[1, 0] * s, Xp * m[1, 1] * s)
    gu, gp = torch.autograd.grad(lu + lp, (Xu, Xp))
    return lu.item(), lp.item(), gu, gp


def rand_rows(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(DEV), torch.randn(n, d, generator=g).to(DEV)


def rand_masks(n, d, seed, p=0.2):
    g = torch.Generator().manual_seed(seed + 1)
    return (torch.rand(2, 2, n, d, generator=g) >= p).to(DEV)


@pytest.mark.parametrize('d', WIDTHS)
@pytest.mark.parametrize('n', [1, 2, 15, 17, 2048, 8193, 20000])
def test_kernel_against_float64_injected_and_drawn_masks(d, n):
    from arlib_amd import ops
    Xu, Xp = rand_rows(n, d, 7 * n + d)
    for masks, seed, stream in ((rand_masks(n, d, n + d), 0, 0), (None, 99, n)):
        loss, (Gu, Gp) = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=seed, stream_id=stream, masks=masks)
        ref_masks = masks if masks is not None else torch.from_numpy(hash_view_masks(seed, stream, n, d)).to(DEV)
        lu, lp, gu, gp = ref_term(Xu, Xp, ref_masks)
        got = loss.cpu().numpy()
        assert abs(got[0] - lu) <= 1e-5 * max(1.0, abs(lu)) and abs(got[1] - lp) <= 1e-5 * max(1.0, abs(lp))
        if n == 1:      # one row: the loss is identically 0 and so is its gradient; fp32 leaves rounding residue of cancelled terms
            assert Gu.abs().max().item() < 1e-5 and Gp.abs().max().item() < 1e-5
        else:
            assert close(Gu.cpu().numpy(), gu.cpu().numpy()) and close(Gp.cpu().numpy(), gp.cpu().numpy())


def test_kernel_drawn_masks_equal_numpy_restatement_bit_for_bit():
    from arlib_amd import ops
    n, d = 333, 64
    Xu, Xp = rand_rows(n, d, 5)
    l1, G1 = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=2 ** 61 + 3, stream_id=17)
    l2, G2 = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, masks=torch.from_numpy(hash_view_masks(2 ** 61 + 3, 17, n, d)).to(DEV))
    assert torch.equal(l1, l2) and torch.equal(G1[0], G2[0]) and torch.equal(G1[1], G2[1])
    l3, _ = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=2 ** 61 + 3, stream_id=18)
    assert not torch.equal(l1, l3)


def test_kernel_duplicates_all_dropped_row_and_accumulation():
    from arlib_amd import ops
    n, d = 40, 32
    Xu, Xp = rand_rows(n, d, 11)
    Xu[5:9] = Xu[4]                                                           # duplicate positions: separate rows of the InfoNCE, never merged
    Xp[20:30] = Xp[3]
    masks = rand_masks(n, d, 3)
    masks[0, 0, 7] = False                                                    # an all-dropped row in one view: its normalised view is 0
    masks[1, 1, 2] = False
    G0 = (torch.full((n, d), 0.5, device=DEV), torch.full((n, d), -0.25, device=DEV))
    loss, (Gu, Gp) = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, G=(G0[0].clone(), G0[1].clone()), upstream=3.0, masks=masks)
    lu, lp, gu, gp = ref_term(Xu, Xp, masks)
    assert torch.isfinite(Gu).all() and torch.isfinite(Gp).all()
    assert close(loss.cpu().numpy(), np.array([lu, lp]))
    assert close((Gu - G0[0]).cpu().numpy(), 3.0 * gu.cpu().numpy()) and close((Gp - G0[1]).cpu().numpy(), 3.0 * gp.cpu().numpy())
    assert torch.all(Gu[7][~masks[0, 1, 7]] == 0.5)                           # dropped in both views: the row's G is untouched there


@pytest.mark.parametrize('d', WIDTHS)
def test_kernel_p0_equals_infonce_and_is_deterministic(d):
    from arlib_amd import ops
    n = 1500
    Xu, Xp = rand_rows(n, d, d)
    loss, (Gu, Gp) = ops.ssl_dropout_nce(Xu, Xp, 0.0, 0.2, seed=1, stream_id=2)
    lu, du1, du2 = ops.infonce_fwd_bwd(Xu, Xu, 0.2)
    lp, dp1, dp2 = ops.infonce_fwd_bwd(Xp, Xp, 0.2)
    assert close(loss.cpu().numpy(), torch.cat([lu, lp]).cpu().numpy())
    assert close(Gu.cpu().numpy(), (du1 + du2).cpu().numpy()) and close(Gp.cpu().numpy(), (dp1 + dp2).cpu().numpy())
    for masks in (None, rand_masks(n, d, 1)):
        a = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=5, stream_id=6, masks=masks)
        b = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=5, stream_id=6, masks=masks)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])


def test_kernel_rejects_unsupported_width_and_arguments():
    from arlib_amd import ops, _lib
    for d in (8, 256, 12):
        Xu, Xp = rand_rows(4, d, 1)
        with pytest.raises(ValueError):
            ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2)
    L = _lib.lib()
    Xu, Xp = rand_rows(4, 256, 1)
    G = torch.zeros_like(Xu), torch.zeros_like(Xp)
    loss = torch.zeros(2, device=DEV)
    ws = torch.empty(max(L.arl_ssl_dropout_nce_workspace_bytes(4, 256) // 4, 4), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.arl_ssl_dropout_nce_f32(p(Xu), p(Xp), 4, 256, 0.2, 0.2, 1.0, 0, 0, None, p(G[0]), p(G[1]), p(loss), p(ws), None)
    assert rc == -2                                                           # ARL_E_DIM
    Xu, Xp = rand_rows(4, 64, 1)
    G = torch.zeros_like(Xu), torch.zeros_like(Xp)
    ws = torch.empty(L.arl_ssl_dropout_nce_workspace_bytes(4, 64) // 4, device=DEV)
    for pp, tau in ((1.0, 0.2), (-0.1, 0.2), (0.2, 0.01)):
        rc = L.arl_ssl_dropout_nce_f32(p(Xu), p(Xp), 4, 64, pp, tau, 1.0, 0, 0, None, p(G[0]), p(G[1]), p(loss), p(ws), None)
        assert rc == -4                                                       # ARL_E_ARG
        with pytest.raises(ValueError):
            ops.ssl_dropout_nce(Xu, Xp, pp, tau)
    torch.cuda.synchronize()
    assert torch.count_nonzero(G[0]) == 0 and torch.count_nonzero(G[1]) == 0


# ------------------------------------------------------------------------------------------------ engine and model
def _fresh(emb=64):
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.SSL4Rec import SSL4Rec
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = SSL4Rec(rec_args(emb_size=emb), make_data())
    return rec


def _rule(stream, B, d):
    return torch.from_numpy(rule_view_masks(stream, B, d)).to(DEV)


def ref_step(rec, E0, u, p, n, masks, reg=1e-4, lr=0.005, betas=(0.9, 0.999), eps=1e-8):
    """float64 SSL4Rec step (SSL4Rec.py:58-75 with Adam step 1): LightGCN mean over layers 0..2, BPR + L2 + cl on the propagated rows."""
    U = rec.data.user_num
    A = rec.model.sparse_norm_adj.to_scipy().toarray()
    A = torch.from_numpy(A).double().to(DEV)
    E = E0.double().detach().requires_grad_(True)
    E1 = A @ E
    out = (E + E1 + A @ E1) / 3
    ue, pe, ne = out[u], out[U + p], out[U + n]
    bpr = -torch.log(1e-8 + torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1))).mean()
    l2 = reg * (ue.norm() + pe.norm())
    s = 1.25
    m = masks.double()

    def nce(v1, v2):
        a, b = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
        lg = a @ b.T / 0.2
        return (torch.logsumexp(lg, 1) - lg.diagonal()).mean()
    cl = nce(pe * m[1, 0] * s, pe * m[1, 1] * s) + nce(ue * m[0, 0] * s, ue * m[0, 1] * s)
    (g,) = torch.autograd.grad(bpr + l2 + cl, (E,))
    mm, vv = (1 - betas[0]) * g, (1 - betas[1]) * g * g
    new = E.detach() - lr * (mm / (1 - betas[0])) / ((vv / (1 - betas[1])).sqrt() + eps)
    return bpr.item(), cl.item(), new


def test_fused_step_equals_float64_step_and_autograd_route():
    rec = _fresh()
    model = rec.model.cuda()
    U = rec.data.user_num
    E0 = model._pack().detach().clone()
    g = torch.Generator().manual_seed(3)
    B = 2048
    u = torch.randint(0, U, (B,), generator=g).to(torch.int32).to(DEV)
    p = torch.randint(0, rec.data.item_num, (B,), generator=g).to(torch.int32).to(DEV)
    n = torch.randint(0, rec.data.item_num, (B,), generator=g).to(torch.int32).to(DEV)
    u[:50] = u[0]; p[100:200] = p[1]                                          # duplicate positions
    masks = _rule(0, B, 64)
    bpr, cl, new = ref_step(rec, E0, u.long(), p.long(), n.long(), masks)
    # the autograd route (a copy of the model, torch Adam over the two tables, the same kernel through _DropoutNce)
    rec2 = copy.deepcopy(rec)
    rec2.model.view_masks = lambda s, b, d: masks
    m2 = rec2.model.cuda()
    opt2 = torch.optim.Adam([m2.embedding_dict['user_emb'], m2.embedding_dict['item_emb']], lr=0.005)
    ue, ie = m2()
    loss = rec2._batch_loss(ue[u.long()], ie[p.long()], ie[n.long()], 1e-4) + rec2._extra_loss(m2, u.long(), p.long(), ue, ie)
    opt2.zero_grad(); loss.backward(); opt2.step()
    # the fused step
    eng = model._engine(1e-4, 0.005, 'adam')
    eng.reg = 1e-4
    lo, cl_f = eng.step_ssl4rec(u, p, n, cl_rate=1, masks=masks)
    assert abs(float(lo[0]) - bpr) < 1e-5 and abs(float(cl_f) - cl) < 1e-4 * abs(cl)
    assert abs(float(rec2.last_cl_loss) - cl) < 1e-4 * abs(cl)
    # one Adam step moves every touched entry by ~lr * sign(g): compare the moved tables (entries with |g| ~ 0 may differ by up to lr)
    ref = new.cpu().numpy()
    for got in (model._pack(), m2._pack()):
        diff = np.abs(got.detach().cpu().numpy() - ref)
        assert np.mean(diff < 1e-5) > 0.999 and diff.max() < 0.011


def test_golden_forward_step0_gradients_and_25_fused_steps():
    g = golden('g29_ssl4rec.npz')
    rec = _fresh()
    model = rec.model.cuda()
    U = rec.data.user_num
    with torch.no_grad():
        u, i = model()
    assert close(pick(u, g, 'fwd_user'), g['fwd_user']) and close(pick(i, g, 'fwd_item'), g['fwd_item'])
    towers0 = [t.detach().clone() for t in model.tower_parameters()]
    batches = golden_batches(g)
    # step-0 gradients through the autograd route
    rec0 = copy.deepcopy(rec)
    m0 = rec0.model.cuda()
    m0.view_masks = lambda s, b, d: _rule(s, b, d)
    bu, bp, bn = (torch.from_numpy(x).long().to(DEV) for x in batches[0])
    ue, ie = m0()
    loss = rec0._batch_loss(ue[bu], ie[bp], ie[bn], 1e-4) + rec0._extra_loss(m0, bu, bp, ue, ie)
    loss.backward()
    for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
        assert close(pick(dict(m0.named_parameters())[n].grad, g, 'grad0__' + n), g['grad0__' + n]), n
    # 25 fused steps with the default optimizer (towers included)
    opt = torch.optim.Adam(model.parameters(), lr=0.005)
    assert rec._fusable(opt) == 'adam'
    eng = model._engine(1e-4, 0.005, 'adam')
    eng.reg = 1e-4
    rec._bind_optimizer_state(eng, opt, 'adam')
    model.view_masks = lambda s, b, d: _rule(s, b, d)
    rl, cl = [], []
    for batch in batches:
        bu, bp, bn = (torch.from_numpy(x).to(DEV) for x in batch)
        lo = rec._fused_step(eng, bu, bp, bn)
        rl.append(float(lo[0])); cl.append(float(rec.last_cl_loss))
    assert np.allclose(rl[:3], g['rec_losses'][:3], rtol=1e-5, atol=0) and np.allclose(cl[:3], g['cl_losses'][:3], rtol=1e-5, atol=0)
    assert np.allclose(rl, g['rec_losses'], rtol=1e-3, atol=0) and np.allclose(cl, g['cl_losses'], rtol=1e-3, atol=0)
    params = dict(model.named_parameters())
    for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
        assert close(pick(params[n], g, 'final__' + n), g['final__' + n], tol=1e-2), n
    assert all(torch.equal(a, b) for a, b in zip(towers0, model.tower_parameters()))


def test_train_api_embgrad_adjgrad_and_copies_match_reference_run():
    g = golden('g29_ssl4rec.npz')
    rec = _fresh()
    rec.model.view_masks = lambda s, b, d: _rule(s, b, d)
    with contextlib.redirect_stdout(io.StringIO()):
        ue, ie, ug, ig = rec.train(Epoch=2, evalNum=1, requires_embgrad=True)
        _, measure = rec.test()
    assert random.random() == float(g['api_next_random'][0])
    assert rel_err(pick(ue, g, 'api_user_emb'), g['api_user_emb']) < 1e-2 and rel_err(pick(ie, g, 'api_item_emb'), g['api_item_emb']) < 1e-2
    assert rel_err(pick(ug, g, 'api_usergrad'), g['api_usergrad']) < 1e-2 and rel_err(pick(ig, g, 'api_itemgrad'), g['api_itemgrad']) < 1e-2
    assert rec.bestPerformance[0] == int(g['api_best_epoch'][0])
    got = np.array([float(m.strip().split(':')[1]) for m in measure[1:]])
    assert np.allclose(got, g['api_measure'], rtol=0, atol=2e-3)
    assert rec.model.mask_stream == 44
    rec.model.view_masks = None
    for r in (copy.deepcopy(rec), pickle.loads(pickle.dumps(rec))):
        assert r.model.mask_seed == rec.model.mask_seed and r.model.mask_stream == 44
        assert rel_err(r.model()[0].detach().cpu().numpy(), rec.model()[0].detach().cpu().numpy()) < 1e-6
    rec = _fresh()
    rec.model.view_masks = lambda s, b, d: _rule(s, b, d)
    with contextlib.redirect_stdout(io.StringIO()):
        block = rec.train(Epoch=1, evalNum=1, requires_adjgrad=True)
    assert close(pick(block, g, 'adj_block'), g['adj_block'], tol=1e-3)


def test_default_training_takes_fused_route_prints_and_keeps_towers():
    from arlib_amd import engine
    rec = _fresh()
    model = rec.model.cuda()
    towers0 = [t.detach().clone() for t in model.tower_parameters()]
    calls = {'n': 0}
    orig = engine.PropagationEngine.step_ssl4rec

    def counted(self, *a, **k):
        calls['n'] += 1
        return orig(self, *a, **k)
    engine.PropagationEngine.step_ssl4rec = counted
    try:
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rec.train(Epoch=1, evalNum=1)
    finally:
        engine.PropagationEngine.step_ssl4rec = orig
    assert calls['n'] == 22 and rec.last_train_stats['fused']
    lines = [l for l in buf.getvalue().splitlines() if l.startswith('training:')]
    assert lines and lines[0].startswith('training: 1 batch 0 rec_loss: ') and ' cl_loss ' in lines[0]
    assert all(torch.equal(a, b) for a, b in zip(towers0, model.tower_parameters()))
    assert model.mask_seed is not None and model.mask_stream == 22
    opt = torch.optim.Adam([model.embedding_dict['user_emb'], model.embedding_dict['item_emb']], lr=0.005)
    assert rec._fusable(opt) == 'adam'
    assert rec._fusable(torch.optim.SGD(model.parameters(), lr=0.1)) is None
    assert rec._fusable(torch.optim.Adam(list(model.parameters())[:3] + list(model.parameters())[8:], lr=0.1)) is None


def test_width_outside_kernel_set_takes_dropout_fallback():
    from arlib_amd import ops
    rec = _fresh(emb=12)
    calls = {'n': 0}
    orig = ops.ssl_dropout_nce

    def counted(*a, **k):
        calls['n'] += 1
        return orig(*a, **k)
    ops.ssl_dropout_nce = counted
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            rec.train(Epoch=1, evalNum=1)
    finally:
        ops.ssl_dropout_nce = orig
    assert calls['n'] == 0 and not rec.last_train_stats['fused']
    assert torch.isfinite(rec.model.embedding_dict['user_emb']).all()

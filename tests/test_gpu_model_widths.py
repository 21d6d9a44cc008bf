"""One training step per model at embedding widths off the MFMA kernels' {16, 32, 64, 128}, against float64 models restated here.

Off those widths the models take other routes (NGCF: element-wise kernels + library GEMMs; NCL: the panel form of the structure loss) and the
sparse kernels run their ragged-lane code.  Each test asserts the route it took (call counts on the `ops` functions), builds the float64
model from the model's own definition on a dense float64 normalised adjacency of ml-100k, and compares the loss and the gradient of every
parameter with conftest.close().  Fused routes are read from the state they leave: Adam's first moment after step 1 is (1 - beta1) g, SGD's
update is lr g."""
import numpy as np
import pytest
import torch
from conftest import close, RTOL
from test_host_api import make_data

pytestmark = pytest.mark.gpu

REG, B = 1e-4, 2048
LOSS_TOL = 1e-5


@pytest.fixture(scope='module')
def data():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')
    return make_data()


@pytest.fixture(scope='module')
def A64(data):
    return torch.from_numpy(data.norm_adj.toarray().astype(np.float64))


def batch(data, seed):
    rng = np.random.default_rng(seed)
    u, p, n = rng.integers(0, data.user_num, B), rng.integers(0, data.item_num, B), rng.integers(0, data.item_num, B)
    u[:100] = u[0]; n[1::9] = p[0]                       # a user repeated, an item that is both positive and negative
    return u, p, n


def dev32(*a):
    return [torch.from_numpy(x.astype(np.int32)).cuda() for x in a]


def dev64(*a):
    return [torch.from_numpy(x.astype(np.int64)).cuda() for x in a]


def _counted(f, calls, key):
    def wrapper(*a, **kw):
        calls[key] += 1
        return f(*a, **kw)
    return wrapper


def counting(monkeypatch, names, owner=None):
    """Count the calls of owner.<name> (default: the `ops` module) for each name; the route a step took."""
    if owner is None:
        from arlib_amd import ops as owner
    calls = dict.fromkeys(names, 0)
    for nm in names:
        monkeypatch.setattr(owner, nm, _counted(getattr(owner, nm), calls, nm))
    return calls


def seeded_table(model, seed, scale=0.1):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in ('user_emb', 'item_emb'):
            t = model.embedding_dict[k]
            t.copy_(((torch.rand(t.shape, generator=g) * 2 - 1) * scale).to(t.device))


def bpr64(out, U, u, p, n, reg=REG):
    ue, pe, ne = out[torch.from_numpy(u)], out[U + torch.from_numpy(p)], out[U + torch.from_numpy(n)]
    x = (ue * pe).sum(1) - (ue * ne).sum(1)
    return (-torch.log(1e-7 + torch.sigmoid(x))).mean() + reg * (torch.norm(ue) + torch.norm(pe))


def lightgcn64(A, E0, L, u, p, n, U):
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)
    layers, x = [E], E
    for _ in range(L):
        x = A @ x
        layers.append(x)
    loss = bpr64(torch.stack(layers).mean(0), U, u, p, n)
    loss.backward()
    return loss.item(), E.grad.numpy()


def table(model):
    return torch.cat([model.embedding_dict['user_emb'].detach(), model.embedding_dict['item_emb'].detach()]).cpu().numpy()


def grads(model):
    return np.concatenate([model.embedding_dict['user_emb'].grad.cpu().numpy(), model.embedding_dict['item_emb'].grad.cpu().numpy()])


# ------------------------------------------------------------------------------------------------ LightGCN
@pytest.mark.parametrize('L', [1, 3])
@pytest.mark.parametrize('d', [12, 100, 256])
def test_lightgcn_step_every_route(data, A64, d, L, monkeypatch):
    from arlib_amd import ops
    from arlib_amd.engine import PropagationEngine
    from arlib_amd.recommender.LightGCN import LGCN_Encoder
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss
    U = data.user_num
    u, p, n = batch(data, d + L)
    torch.manual_seed(d)
    model = LGCN_Encoder(data, d, L).cuda()
    seeded_table(model, d)
    E0 = table(model)
    ref_loss, ref_g = lightgcn64(A64, E0, L, u, p, n, U)
    # autograd
    calls = counting(monkeypatch, ['spmm', 'spmm_layersum', 'spmm_rows', 'spmm_flagged', 'spmm_adam', 'bpr_l2_fwd_bwd'])
    ue, ie = model()
    uu, pp, nn_ = dev64(u, p, n)
    loss = bpr_loss(ue[uu], ie[pp], ie[nn_]) + l2_reg_loss(REG, ue[uu], ie[pp])
    loss.backward()
    assert calls['spmm'] + calls['spmm_layersum'] == 2 * L and calls['spmm_rows'] == 0 and calls['bpr_l2_fwd_bwd'] > 0
    assert abs(loss.item() - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close(grads(model), ref_g)
    # fused sparse step (Adam only): the gradient is the first moment / (1 - beta1)
    calls.update(dict.fromkeys(calls, 0))
    eng = model._engine()
    eng.reg, eng.lr = REG, 0.005                                    # the engine the forward built (reg, lr = 0) is the one the fused route reuses
    assert eng.t == 0 and float(eng.m.abs().max()) == 0.0
    lo = eng.step(*dev32(u, p, n))
    assert calls['spmm_rows'] == 1 and calls['spmm_flagged'] >= 1 and (calls['spmm_adam'] == 1) == (L > 1)
    assert abs(float(lo[0] + lo[1]) - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close(eng.m.cpu().numpy() / (1 - eng.betas[0]), ref_g)
    # step_dense with SGD: g = (E0 - E1) / lr, lr large enough that lr |g| dominates |E0| in fp32
    lr = 1e6                                                        # lr |g| >> |E0| on every row above close()'s 1e-3 row floor
    calls.update(dict.fromkeys(calls, 0))
    sgd = PropagationEngine(model._graph(), U, data.item_num, d, L, REG, lr, 'cuda:0', optimizer='sgd', table=torch.from_numpy(E0).cuda())
    lo = sgd.step(*dev32(u, p, n))
    assert calls['spmm'] + calls['spmm_layersum'] == 2 * L and calls['spmm_rows'] == 0 and calls['spmm_flagged'] == 0
    assert abs(float(lo[0] + lo[1]) - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close((E0.astype(np.float64) - sgd.E0.cpu().numpy()) / lr, ref_g)


@pytest.mark.parametrize('d', [50, 260])
def test_lightgcn_refuses_unsupported_width_before_launch(data, d, monkeypatch):
    from arlib_amd import ops, _lib
    from arlib_amd.engine import PropagationEngine
    from arlib_amd.recommender.LightGCN import LGCN_Encoder
    model = LGCN_Encoder(data, d, 2).cuda()
    calls = counting(monkeypatch, list(_lib.EXPORTS), owner=_lib.lib())     # every entry of the C ABI: nothing may be called
    with pytest.raises(ValueError, match='embedding size %d unsupported' % d):
        model()
    with pytest.raises(ValueError, match='embedding size %d unsupported' % d):
        PropagationEngine(model._graph(), data.user_num, data.item_num, d, 2, REG, 0.005, 'cuda:0')
    assert sum(calls.values()) == 0, {k: v for k, v in calls.items() if v}


# ------------------------------------------------------------------------------------------------ GMF (no propagation)
@pytest.mark.parametrize('d', [12, 50, 100, 256])
def test_gmf_step_autograd_and_fused(data, A64, d, monkeypatch):
    from types import SimpleNamespace
    from arlib_amd.engine import PropagationEngine
    from arlib_amd.recommender.GMF import GMF
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss
    U = data.user_num
    u, p, n = batch(data, d)
    args = SimpleNamespace(dataset='ml-100k', model_name='GMF', maxEpoch=1, batch_size=B, emb_size=d, n_layers=0, reg=REG, lRate=0.005, seed=2018, topK='50')
    model = GMF(args, data).model.cuda()
    seeded_table(model, d, 0.5)
    E0 = table(model)
    ref_loss, ref_g = lightgcn64(A64, E0, 0, u, p, n, U)
    calls = counting(monkeypatch, ['bpr_l2_fwd_bwd', 'adam_dense', 'spmm'])
    ue, ie = model()
    uu, pp, nn_ = dev64(u, p, n)
    loss = bpr_loss(ue[uu], ie[pp], ie[nn_]) + l2_reg_loss(REG, ue[uu], ie[pp])
    loss.backward()
    assert abs(loss.item() - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close(grads(model), ref_g)
    eng = PropagationEngine(None, U, data.item_num, d, 0, REG, 0.005, 'cuda:0', table=torch.from_numpy(E0).cuda())
    lo = eng.step(*dev32(u, p, n))                                  # L = 0: step_dense
    assert calls['adam_dense'] == 1 and calls['spmm'] == 0
    assert abs(float(lo[0] + lo[1]) - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close(eng.m.cpu().numpy() / (1 - eng.betas[0]), ref_g)


# ------------------------------------------------------------------------------------------------ NGCF off NGCF_DENSE_WIDTHS
def ngcf64(A, E0, Ws, L, u, p, n, U, slope=0.01):
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)
    W = [torch.tensor(w, dtype=torch.float64, requires_grad=True) for w in Ws]
    layers, x = [E], E
    for k in range(L):
        P = A @ x
        x = torch.nn.functional.leaky_relu((P + x) @ W[2 * k] + (P * x) @ W[2 * k + 1], slope)
        layers.append(x)
    loss = bpr64(torch.stack(layers).mean(0), U, u, p, n)
    loss.backward()
    return loss.item(), E.grad.numpy(), [w.grad.numpy() for w in W]


@pytest.mark.parametrize('rows_form', [False, True])
@pytest.mark.parametrize('d', [12, 100, 256])
def test_ngcf_layers_off_mfma_widths(data, A64, d, rows_form, monkeypatch):
    """_Layer (full forward) and _LastLayerRows (training forward) at widths without the MFMA dense kernels."""
    from arlib_amd import ops
    from arlib_amd.recommender.NGCF import NGCF_Encoder
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss
    L, U = 2, data.user_num
    assert d not in ops.NGCF_DENSE_WIDTHS
    u, p, n = batch(data, d + 7)
    torch.manual_seed(d)
    model = NGCF_Encoder(data, d, L).cuda()
    seeded_table(model, d)
    E0 = table(model)
    names = [k % l for l in range(L) for k in ('w1_%d', 'w2_%d')]
    Ws = [model.W[k].detach().cpu().numpy() for k in names]
    ref_loss, ref_g, ref_W = ngcf64(A64, E0, Ws, L, u, p, n, U)
    calls = counting(monkeypatch, ['ngcf_combine', 'ngcf_act_', 'ngcf_act_bwd', 'ngcf_combine_bwd', 'ngcf_dense_fwd', 'ngcf_dense_bwd'])
    if rows_form:
        out = model.forward_rows(torch.cat(dev32(u, p + U, n + U)))
        ue, pe, ne = out[:B], out[B:2 * B], out[2 * B:]
    else:
        fu, fi = model()
        uu, pp, nn_ = dev64(u, p, n)
        ue, pe, ne = fu[uu], fi[pp], fi[nn_]
    loss = bpr_loss(ue, pe, ne) + l2_reg_loss(REG, ue, pe)
    loss.backward()
    assert calls['ngcf_dense_fwd'] == 0 and calls['ngcf_dense_bwd'] == 0
    assert all(calls[k] == L for k in ('ngcf_combine', 'ngcf_act_', 'ngcf_act_bwd', 'ngcf_combine_bwd')), calls
    assert abs(loss.item() - ref_loss) <= LOSS_TOL * abs(ref_loss)
    assert close(grads(model), ref_g)
    for k, rw in zip(names, ref_W):
        assert close(model.W[k].grad.cpu().numpy(), rw), k


# ------------------------------------------------------------------------------------------------ NCL's structure loss, panel form
@pytest.mark.parametrize('d,tau', [(100, 0.05), (64, 0.02)])
def test_ncl_structure_loss_panel_form(data, d, tau, monkeypatch):
    from arlib_amd import ops
    from arlib_amd.recommender import NCL
    from arlib_amd.recommender.NCL import all_rows_nce
    assert d not in ops.NCE_ALLROWS_WIDTHS or tau < ops.NCE_ALLROWS_MIN_TAU
    calls = counting(monkeypatch, ['nce_allrows', 'normalize_rows'])
    panel = counting(monkeypatch, ['forward'], owner=NCL._AllRowsNCE)
    monkeypatch.setattr(NCL._AllRowsNCE, 'PANEL', 512)                # several panels: the running maximum carries across them
    g = torch.Generator().manual_seed(d)
    Nv, nA = data.item_num, 700
    Xv = torch.randn(Nv, d, generator=g) * 0.3
    idx = torch.randint(0, Nv, (nA,), generator=g)
    Xa = Xv[idx] + torch.randn(nA, d, generator=g)               # positives not so close that every term of the loss cancels to ~0
    a, v = Xa.cuda().requires_grad_(), Xv.cuda().requires_grad_()
    loss = all_rows_nce(a, v, idx.cuda(), tau)
    loss.backward()
    assert calls['nce_allrows'] == 0 and calls['normalize_rows'] == 0 and panel['forward'] == 1
    a64, v64 = Xa.double().requires_grad_(), Xv.double().requires_grad_()
    an, vn = torch.nn.functional.normalize(a64, dim=1), torch.nn.functional.normalize(v64, dim=1)
    S = an @ vn.T / tau
    ref = (torch.logsumexp(S, 1) - S[torch.arange(nA), idx]).sum()
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item())
    # at tau = 0.02 the logits reach 50 and the batch-side gradient's rows are differences of softmax-weighted sums projected off their own
    # direction: the same panel expression evaluated in fp32 on the CPU is 2-4e-4 row-wise from float64 on some rows (max-norm 1.3e-6), so
    # the row-wise bar is 1e-3 below NCE_ALLROWS_MIN_TAU; the max-norm bar stays RTOL
    row_tol = RTOL if tau >= ops.NCE_ALLROWS_MIN_TAU else 1e-3
    assert close(a.grad.cpu().numpy(), a64.grad.numpy(), row_tol=row_tol) and close(v.grad.cpu().numpy(), v64.grad.numpy(), row_tol=row_tol)


# ------------------------------------------------------------------------------------------------ WRMF
@pytest.mark.parametrize('d', [4, 256, 257])
def test_wrmf_step_autograd(data, d, monkeypatch):
    from types import SimpleNamespace
    from arlib_amd.recommender.WRMF import WRMF
    from arlib_amd.util.loss import wrmf_l2_loss
    U = data.user_num
    u, p, n = batch(data, d + 3)
    args = SimpleNamespace(dataset='ml-100k', model_name='WRMF', maxEpoch=1, batch_size=B, emb_size=d, n_layers=0, reg=REG, lRate=0.005, seed=2018, topK='50')
    rec = WRMF(args, data)
    model = rec.model.cuda()
    seeded_table(model, d, 0.5 / np.sqrt(d))
    E0 = table(model)
    calls = counting(monkeypatch, ['wrmf_l2_fwd_bwd', 'bpr_l2_fwd_bwd'])
    ue, ie = model()
    uu, pp, nn_ = dev64(u, p, n)
    loss = rec._batch_loss(ue[uu], ie[pp], ie[nn_], REG)
    loss.backward()
    assert calls['wrmf_l2_fwd_bwd'] == 2 and calls['bpr_l2_fwd_bwd'] == 0
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)
    ue, pe, ne = E[torch.from_numpy(u)], E[U + torch.from_numpy(p)], E[U + torch.from_numpy(n)]
    ref = (20 * ((ue * pe).sum(1) - 1) ** 2 + (ue * ne).sum(1) ** 2).sum() + REG * (torch.norm(ue) + torch.norm(pe))
    ref.backward()
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item())
    assert close(grads(model), E.grad.numpy())


# ------------------------------------------------------------------------------------------------ SimGCL, XSimGCL, SGL: fused Adam steps
def csr_graph(M):
    from arlib_amd import ops
    M = M.tocsr().astype(np.float32)
    M.sort_indices()
    return ops.CSRGraph(M.indptr.astype(np.int64), M.indices.astype(np.int32), M.data, 'cuda:0')


def infonce64(a, b, tau):
    an, bn = torch.nn.functional.normalize(a, dim=1), torch.nn.functional.normalize(b, dim=1)
    S = an @ bn.T / tau
    return (torch.logsumexp(S, 1) - S.diagonal()).mean()


def perturb64(x, noise, eps):
    return x + torch.sign(x) * torch.nn.functional.normalize(torch.from_numpy(noise.astype(np.float64)), dim=1) * eps


def cl_rows(u, p, U):
    return torch.from_numpy(np.unique(u)), torch.from_numpy(np.unique(p) + U)


def check_fused_step(eng, lo, cl, ref_rec, ref_cl, ref_g):
    assert abs(float(lo[0] + lo[1]) - ref_rec) <= LOSS_TOL * abs(ref_rec)
    assert abs(float(cl) - ref_cl) <= LOSS_TOL * abs(ref_cl)
    assert eng.t == 1
    assert close(eng.m.cpu().numpy() / (1 - eng.betas[0]), ref_g)            # Adam's first moment after one step: (1 - beta1) g


@pytest.mark.parametrize('d', [100, 256])
def test_simgcl_fused_step(data, A64, d, monkeypatch):
    """engine.step_simgcl with injected noise: clean forward for BPR + L2, two perturbed views for the InfoNCE of the batch's unique users and
    unique positive items, layer 0 left out of the mean (recommender/SimGCL.py)."""
    from arlib_amd.engine import PropagationEngine
    U, L, cl_rate, tau, eps = data.user_num, 2, 0.2, 0.2, 0.1
    u, p, n = batch(data, d + 11)
    rng = np.random.default_rng(d)
    N = U + data.item_num
    E0 = ((rng.random((N, d)) * 2 - 1) * 0.1).astype(np.float32)
    noises = [[rng.random((N, d)).astype(np.float32) for _ in range(L)] for _ in range(2)]
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)

    def forward(view):
        x, layers = E, []
        for k in range(L):
            x = A64 @ x
            if view is not None:
                x = perturb64(x, noises[view][k], eps)
            layers.append(x)
        return torch.stack(layers).mean(0)
    rec = bpr64(forward(None), U, u, p, n)
    v1, v2 = forward(0), forward(1)
    uu, ii = cl_rows(u, p, U)
    cl = cl_rate * (infonce64(v1[uu], v2[uu], tau) + infonce64(v1[ii], v2[ii], tau))
    (rec + cl).backward()
    calls = counting(monkeypatch, ['spmm_rows', 'spmm_flagged', 'simgcl_perturb_', 'simgcl_perturb_rng', 'infonce_fwd_bwd'])
    eng = PropagationEngine(csr_graph(data.norm_adj), U, data.item_num, d, L, REG, 0.005, 'cuda:0', skip_layer0=True, table=torch.from_numpy(E0).cuda())
    lo, cl_out = eng.step_simgcl(*dev32(u, p, n), cl_rate=cl_rate, tau=tau, eps=eps, noises=[[torch.from_numpy(x).cuda() for x in v] for v in noises])
    assert calls['spmm_rows'] == 3 and calls['spmm_flagged'] >= 1 and calls['infonce_fwd_bwd'] == 2
    assert calls['simgcl_perturb_'] == 2 * L and calls['simgcl_perturb_rng'] == 0
    check_fused_step(eng, lo, cl_out, rec.item(), cl.item(), E.grad.numpy())


@pytest.mark.parametrize('layer_cl', [1, 2])
@pytest.mark.parametrize('d', [100, 256])
def test_xsimgcl_fused_step(data, A64, d, layer_cl, monkeypatch):
    """engine.step_xsimgcl with injected noise: one perturbed forward, BPR + L2 on the mean of layers 1..L, InfoNCE between that mean and the
    layer-`layer_cl` output (recommender/XSimGCL.py)."""
    from arlib_amd.engine import PropagationEngine
    U, L, cl_rate, tau, eps = data.user_num, 2, 0.2, 0.2, 0.1
    u, p, n = batch(data, d + 13)
    rng = np.random.default_rng(d + layer_cl)
    N = U + data.item_num
    E0 = ((rng.random((N, d)) * 2 - 1) * 0.1).astype(np.float32)
    noises = [rng.random((N, d)).astype(np.float32) for _ in range(L)]
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)
    x, layers = E, []
    for k in range(L):
        x = perturb64(A64 @ x, noises[k], eps)
        layers.append(x)
    mean = torch.stack(layers).mean(0)
    rec = bpr64(mean, U, u, p, n)
    uu, ii = cl_rows(u, p, U)
    lay = layers[layer_cl - 1]
    cl = cl_rate * (infonce64(mean[uu], lay[uu], tau) + infonce64(mean[ii], lay[ii], tau))
    (rec + cl).backward()
    calls = counting(monkeypatch, ['spmm_rows', 'spmm_flagged', 'spmm_adam', 'infonce_fwd_bwd'])
    eng = PropagationEngine(csr_graph(data.norm_adj), U, data.item_num, d, L, REG, 0.005, 'cuda:0', skip_layer0=True, table=torch.from_numpy(E0).cuda())
    lo, cl_out = eng.step_xsimgcl(*dev32(u, p, n), cl_rate=cl_rate, tau=tau, eps=eps, layer_cl=layer_cl, noises=[torch.from_numpy(x).cuda() for x in noises])
    assert calls['spmm_rows'] == 1 and calls['spmm_flagged'] >= 1 and calls['spmm_adam'] == 1 and calls['infonce_fwd_bwd'] == 2
    check_fused_step(eng, lo, cl_out, rec.item(), cl.item(), E.grad.numpy())


@pytest.mark.parametrize('d', [100])
def test_sgl_fused_step(data, A64, d, monkeypatch):
    """engine.step_sgl: BPR + L2 on the clean graph, one InfoNCE over the batch's unique users and items between two edge-dropped views
    (recommender/SGL.py), the three passes' gradients summed into one Adam step."""
    from arlib_amd.engine import PropagationEngine
    from oracle import oracle as O
    U, I, L, cl_rate, tau = data.user_num, data.item_num, 2, 0.2, 0.2
    u, p, n = batch(data, d + 17)
    rng = np.random.default_rng(d)
    R = data.norm_adj.tocoo()
    keep = (R.row < U) & (R.col >= U)
    pu, pi = R.row[keep], R.col[keep] - U
    views, views64 = [], []
    for _ in range(2):                                                   # edge dropout (ratio 0.1), renormalised
        k = rng.random(len(pu)) >= 0.1
        rowptr, col, w = O.bipartite_csr(pu[k], pi[k], U, I)
        val = O.norm_adj_values(rowptr, col, w)
        M = sp_csr(rowptr, col, val, U + I)
        views.append(csr_graph(M))
        views64.append(torch.from_numpy(M.toarray().astype(np.float64)))
    E0 = ((rng.random((U + I, d)) * 2 - 1) * 0.1).astype(np.float32)
    E = torch.tensor(E0, dtype=torch.float64, requires_grad=True)

    def lightgcn(Ag):
        x, layers = E, [E]
        for _ in range(L):
            x = Ag @ x
            layers.append(x)
        return torch.stack(layers).mean(0)
    rec = bpr64(lightgcn(A64), U, u, p, n)
    uu, ii = cl_rows(u, p, U)
    rc = torch.cat([uu, ii])
    cl = cl_rate * infonce64(lightgcn(views64[0])[rc], lightgcn(views64[1])[rc], tau)
    (rec + cl).backward()
    calls = counting(monkeypatch, ['spmm_rows', 'spmm_flagged', 'infonce_fwd_bwd', 'adam_dense'])
    eng = PropagationEngine(csr_graph(data.norm_adj), U, I, d, L, REG, 0.005, 'cuda:0', table=torch.from_numpy(E0).cuda())
    lo, cl_out = eng.step_sgl(*dev32(u, p, n), views[0], views[1], cl_rate=cl_rate, tau=tau)
    assert calls['spmm_rows'] == 3 and calls['spmm_flagged'] == 3 * L and calls['infonce_fwd_bwd'] == 1 and calls['adam_dense'] == 1
    check_fused_step(eng, lo, cl_out, rec.item(), cl.item(), E.grad.numpy())


def sp_csr(rowptr, col, val, n):
    import scipy.sparse as sp
    return sp.csr_matrix((val, col, rowptr), shape=(n, n))


# ------------------------------------------------------------------------------------------------ NCF off NCF_TOWER_WIDTHS
@pytest.mark.parametrize('rows_form', [False, True])
@pytest.mark.parametrize('d', [48, 100])
def test_ncf_torch_tower_step(data, d, rows_form, monkeypatch):
    """NCF at widths without the fused tower kernel: the tower runs on nn.Linear; loss and the gradient of every table and weight against
    float64."""
    from types import SimpleNamespace
    from arlib_amd import ops
    from arlib_amd.recommender.NCF import NCF
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss
    assert d not in ops.NCF_TOWER_WIDTHS
    U = data.user_num
    u, p, n = batch(data, d + 19)
    args = SimpleNamespace(dataset='ml-100k', model_name='NCF', maxEpoch=1, batch_size=B, emb_size=d, n_layers=0, reg=REG, lRate=0.005, seed=2018, topK='50')
    torch.manual_seed(d)
    model = NCF(args, data).model.cuda()
    names = ['user_mf_emb', 'item_mf_emb', 'user_mlp_emb', 'item_mlp_emb']
    T64 = {k: model.embedding_dict[k].detach().cpu().double().requires_grad_() for k in names}
    W64 = [w.detach().cpu().double().requires_grad_() for w in model._weights()]

    def tower(x):
        for k in range(3):
            x = torch.relu(x @ W64[2 * k].T + W64[2 * k + 1])
        return x
    ui, pi_, ni = (torch.from_numpy(x) for x in (u, p, n))
    ue = torch.cat([T64['user_mf_emb'][ui], tower(T64['user_mlp_emb'][ui])], 1)
    pe = torch.cat([T64['item_mf_emb'][pi_], tower(T64['item_mlp_emb'][pi_])], 1)
    ne = torch.cat([T64['item_mf_emb'][ni], tower(T64['item_mlp_emb'][ni])], 1)
    x = (ue * pe).sum(1) - (ue * ne).sum(1)
    ref = (-torch.log(1e-7 + torch.sigmoid(x))).mean() + REG * (torch.norm(ue) + torch.norm(pe))
    ref.backward()
    calls = counting(monkeypatch, ['ncf_tower_fwd', 'ncf_tower_bwd', 'bpr_l2_fwd_bwd'])
    if rows_form:
        out = model.forward_rows(torch.cat(dev32(u, p + U, n + U)))
        ue, pe, ne = out[:B], out[B:2 * B], out[2 * B:]
    else:
        fu, fi = model()
        uu, pp, nn_ = dev64(u, p, n)
        ue, pe, ne = fu[uu], fi[pp], fi[nn_]
    loss = bpr_loss(ue, pe, ne) + l2_reg_loss(REG, ue, pe)
    loss.backward()
    assert calls['ncf_tower_fwd'] == 0 and calls['ncf_tower_bwd'] == 0 and calls['bpr_l2_fwd_bwd'] > 0
    assert abs(loss.item() - ref.item()) <= LOSS_TOL * abs(ref.item())
    for k in names:
        assert close(model.embedding_dict[k].grad.cpu().numpy(), T64[k].grad.numpy()), k
    for w, w64 in zip(model._weights(), W64):
        assert close(w.grad.cpu().numpy(), w64.grad.numpy())

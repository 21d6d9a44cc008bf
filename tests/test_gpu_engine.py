"""GPU parity: the fused training engine against the golden training runs captured from the reference
(LightGCN/GMF Adam, LightGCN SGD, SimGCL forward) and against the oracle on a synthetic graph."""
import numpy as np
import pytest
import torch
from conftest import golden, rel_err, close, RTOL
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def mods():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')
    from arlib_amd import ops, engine
    return ops, engine


def ml_graph(ops, ml100k):
    p = ml100k['pairs0']
    rowptr, col, w = O.bipartite_csr(p[:, 0], p[:, 1], ml100k['U'], ml100k['I'])
    val, _ = ops.norm_adj_values(T(rowptr.astype(np.int32)), T(col), T(w), len(rowptr) - 1)     # device normalisation
    return ops.CSRGraph(rowptr, col, val, DEV)


def run_golden(mods, ml100k, g, L, lr, opt, snaps):
    ops, engine = mods
    U, I = ml100k['U'], ml100k['I']
    A = ml_graph(ops, ml100k) if L > 0 else None
    d = g['user0'].shape[1]
    eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, lr, DEV, optimizer=opt, table=T(np.concatenate([g['user0'], g['item0']])))
    off = np.concatenate([[0], np.cumsum(g['batch_sizes'])])
    for k in range(len(g['batch_sizes'])):
        sl = slice(off[k], off[k + 1])
        u, p, n = T(g['batch_u'][sl]), T(g['batch_p'][sl]), T(g['batch_n'][sl])
        if k == 0:
            lo, grad = eng.grad(u, p, n)
            gr = grad.cpu().numpy()
            assert close(gr[:U], g['grad_user_step0']) and close(gr[U:], g['grad_item_step0'])
        lo = eng.step(u, p, n).cpu().numpy()
        assert abs(lo[0] + lo[1] - g['losses'][k]) <= RTOL * abs(g['losses'][k])
        if (k + 1) in snaps:
            E = eng.E0.cpu().numpy()
            assert close(E[:U], g['user_k%d' % (k + 1)]) and close(E[U:], g['item_k%d' % (k + 1)])
    return eng


def test_lightgcn_adam_golden_10_steps(mods, ml100k):
    g = golden('g5_lightgcn_adam.npz')
    eng = run_golden(mods, ml100k, g, 3, 0.005, 'adam', {1, 3, 10})
    U = ml100k['U']
    assert close(eng.m[:U].cpu().numpy(), g['m_user']) and close(eng.v[U:].cpu().numpy(), g['v_item'])


def test_gmf_adam_golden_25_steps(mods, ml100k):
    g = golden('g5_gmf_adam.npz')
    eng = run_golden(mods, ml100k, g, 0, 0.005, 'adam', {3, 25})
    U = ml100k['U']
    assert close(eng.m[U:].cpu().numpy(), g['m_item']) and close(eng.v[:U].cpu().numpy(), g['v_user'])


def test_lightgcn_sgd_golden(mods, ml100k):
    run_golden(mods, ml100k, golden('g5_lightgcn_sgd.npz'), 2, 0.0005, 'sgd', {3})


@pytest.mark.parametrize('L', [1, 2, 3])
def test_lightgcn_forward_golden(mods, ml100k, L):
    ops, engine = mods
    g = golden('g4_forward.npz')
    U, I = ml100k['U'], ml100k['I']
    eng = engine.PropagationEngine(ml_graph(ops, ml100k), U, I, 32, L, 1e-4, 0.005, DEV, table=T(np.concatenate([g['lgn_user0'], g['lgn_item0']])))
    out = eng.forward().cpu().numpy()
    assert close(out[:U], g['lgn_L%d_user' % L]) and close(out[U:], g['lgn_L%d_item' % L])


def test_simgcl_forward_and_backward_golden(mods, ml100k):
    ops, engine = mods
    g = golden('g5_simgcl.npz')
    U, I = ml100k['U'], ml100k['I']
    E0 = np.concatenate([g['user0'], g['item0']])
    eng = engine.PropagationEngine(ml_graph(ops, ml100k), U, I, 16, 2, 1e-4, 0.005, DEV, skip_layer0=True, table=T(E0))
    out = eng.forward().cpu().numpy()
    assert close(out[:U], g['fwd_user']) and close(out[U:], g['fwd_item'])
    outp = eng.forward(noises=[T(g['noise'][0]), T(g['noise'][1])], eps=0.1).cpu().numpy()
    assert close(outp[:U], g['fwdp_user']) and close(outp[U:], g['fwdp_item'])
    # backward of the skip-0 mean against the oracle's Horner restatement
    rng = np.random.default_rng(0)
    G = np.zeros_like(E0); rows = rng.integers(0, U + I, 500); G[rows] = rng.standard_normal((500, 16)).astype(np.float32)
    p = ml100k['pairs0']
    rowptr, col, w = O.bipartite_csr(p[:, 0], p[:, 1], U, I)
    csr = (rowptr, col, O.norm_adj_values(rowptr, col, w))
    ref = O.lightgcn_backward(csr, G, 2, skip0=True)
    got = eng.backward_to_table(T(G)).cpu().numpy()
    assert rel_err(got, ref) < RTOL


@pytest.mark.parametrize('schedule', ['csr', 'blocked'])
def test_engine_vs_oracle_synthetic_long_rows(mods, schedule):
    """Synthetic power-law graph with rows far longer than the chunk size, 5 Adam steps vs the oracle; full hops through the
    row-per-group CSR kernel or the register-blocked schedule (with split rows above its threshold)."""
    ops, engine = mods
    rng = np.random.default_rng(42)
    U, I, d, L, B = 20000, 2000, 64, 3, 2048
    deg = np.clip(np.round(np.exp(rng.normal(np.log(16) - 0.5, 1.0, U))), 2, 500).astype(np.int64)
    us = np.repeat(np.arange(U), deg)
    its = np.floor(I * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    val = O.norm_adj_values(rowptr, col, w)
    assert np.diff(rowptr).max() > 2000
    A = ops.CSRGraph(rowptr, col, val, DEV)
    bound = np.sqrt(6.0 / (U + d))
    E0 = ((rng.random((U + I, d)) * 2 - 1) * bound).astype(np.float32)
    st = O.TrainState(E0[:U], E0[U:], (rowptr, col, val), L, 1e-4, 0.005)
    eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, DEV, table=T(E0), schedule=schedule)
    assert (A.blocked is not None) == (schedule == 'blocked') and (schedule == 'csr' or sum(s_['n_split'] for s_ in A.blocked.sets) > 0)
    pairs = np.stack([us, its], 1)
    for k in range(5):
        sel = rng.integers(0, len(pairs), B)
        bu, bp = pairs[sel, 0].copy(), pairs[sel, 1].copy()
        bn = rng.integers(0, I, B).astype(np.int32)
        loss = st.step(bu, bp, bn)
        lo = eng.step(T(bu), T(bp), T(bn)).cpu().numpy()
        assert abs(lo[0] + lo[1] - loss) <= RTOL * abs(loss)
    assert rel_err(eng.E0.cpu().numpy(), st.E0) < RTOL
    assert rel_err(eng.m.cpu().numpy(), st.m) < RTOL and rel_err(eng.v.cpu().numpy(), st.v) < RTOL


def test_sparse_step_equals_dense_step(mods):
    """The sparse-batch step (row-subset last hop, flag-masked first backward hop) must reproduce the dense 2L-hop step."""
    ops, engine = mods
    rng = np.random.default_rng(9)
    U, I, d, B = 6000, 800, 64, 512
    us = np.repeat(np.arange(U), 10)
    its = np.floor(I * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    val = O.norm_adj_values(rowptr, col, w)
    assert np.diff(rowptr).max() > 1500                                   # hot items: long rows in the subset hop too
    E0 = ((rng.random((U + I, d)) * 2 - 1) * 0.05).astype(np.float32)
    for L in (1, 2, 3, 4):
        A = ops.CSRGraph(rowptr, col, val, DEV)
        ea = engine.PropagationEngine(ops.CSRGraph(rowptr, col, val, DEV), U, I, d, L, 1e-4, 0.005, DEV, table=T(E0), schedule='blocked' if L % 2 else 'csr')
        eb = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, DEV, table=T(E0))
        assert A.blocked is None and (ea.A.blocked is not None) == bool(L % 2)
        for k in range(4):
            sel = rng.integers(0, len(us), B)
            bu, bp, bn = T(us[sel].copy()), T(its[sel].copy()), T(rng.integers(0, I, B).astype(np.int32))
            if k == 2:
                bu[:50] = bu[0]; bp[:80] = bp[1]; bn[:30] = bp[1]            # heavy duplicates, item both positive and negative
            la = ea.step(bu, bp, bn).cpu().numpy()
            lb = eb.step_dense(bu, bp, bn).cpu().numpy()
            assert np.allclose(la, lb, rtol=RTOL, atol=0), (L, k)
        assert rel_err(ea.E0.cpu().numpy(), eb.E0.cpu().numpy()) < RTOL, L
        assert rel_err(ea.m.cpu().numpy(), eb.m.cpu().numpy()) < RTOL and rel_err(ea.v.cpu().numpy(), eb.v.cpu().numpy()) < RTOL
        assert float(ea.G.abs().max()) == 0.0 and int(ea.flags.max()) == 0 and int(ea.bits.abs().max()) == 0       # sparse state is cleared after every step
        assert int(ea.dup_bits.abs().max()) == 0                                                                     # the duplicate bitmap too


@pytest.mark.parametrize('d', [32, 8, 128, 256])          # 256: one row per wave, the flag mask needs all 64 lanes (found by tools/spmm_fuzz.py)
def test_spmm_rows_and_flagged_primitives(mods, d):
    ops, engine = mods
    rng = np.random.default_rng(10)
    U, I = 3000, 500
    us = np.repeat(np.arange(U), 8)
    its = np.floor(I * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w = O.bipartite_csr(us, its, U, I)
    val = O.norm_adj_values(rowptr, col, w)
    csr = (rowptr, col, val)
    A = ops.CSRGraph(rowptr, col, val, DEV)
    N = U + I
    X = rng.standard_normal((N, d)).astype(np.float32); L1 = rng.standard_normal((N, d)).astype(np.float32)
    rows = np.concatenate([rng.integers(0, N, 700), [U, U, U + 1, 0]]).astype(np.int32)     # hottest items, duplicates
    ref = 0.25 * (X[rows] + L1[rows] + O.spmm(csr, X)[rows])
    for ns in (1, 16, 33):
        got = ops.spmm_rows(A, T(X), T(rows), [T(X), T(L1)], 0.25, nsplit=ns).cpu().numpy()
        assert rel_err(got, ref) < RTOL
    Gs = np.zeros((N, d), np.float32)
    nz = rng.choice(N, 300, replace=False); nz[:3] = [U, U + 1, 5]
    Gs[nz] = rng.standard_normal((300, d)).astype(np.float32)
    flags = np.zeros(N, np.uint8); flags[nz] = 1
    ref = O.spmm(csr, Gs, 1.0, 1.0, Gs)
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=DEV)
    ops.mark_bits_(bits, T(np.concatenate([nz, nz[:7]]).astype(np.int32)), True, N)
    bn = bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(((bn[np.arange(N) >> 5] >> (np.arange(N) & 31)) & 1).astype(np.uint8), flags)
    got = ops.spmm_flagged(A, T(Gs), bits, 1.0, 1.0, T(Gs), T(flags)).cpu().numpy()
    assert rel_err(got, ref) < RTOL
    got2 = ops.spmm_flagged(A, T(X), None, 0.5, 0.5, T(Gs), T(flags)).cpu().numpy()
    assert rel_err(got2, O.spmm(csr, X, 0.5, 0.5, Gs)) < RTOL
    f = torch.zeros(N, dtype=torch.uint8, device=DEV)
    ops.mark_rows_(f, T(nz.astype(np.int32)), 1)
    assert np.array_equal(f.cpu().numpy(), flags)
    ops.mark_bits_(bits, T(nz.astype(np.int32)), False, N)
    assert int(bits.abs().max()) == 0
    Z = T(Gs.copy()); ops.zero_rows_(Z, T(nz.astype(np.int32)))
    assert float(Z.abs().max()) == 0.0


def test_simgcl_fused_step_matches_reference(mods, ml100k):
    """Fused SimGCL step (shared first hop, row-subset last hops, ONE backward pass for the three forwards) against the
    reference's step with the same injected noise: losses, and tables after the Adam update."""
    ops, engine = mods
    g = golden('g5_simgcl.npz')
    U, I = ml100k['U'], ml100k['I']
    E0 = np.concatenate([g['user0'], g['item0']])
    eng = engine.PropagationEngine(ml_graph(ops, ml100k), U, I, 16, 2, 1e-4, 0.005, DEV, skip_layer0=True, table=T(E0))
    noise = [T(x) for x in g['noise']]
    lo, cl = eng.step_simgcl(T(g['batch_u']), T(g['batch_p']), T(g['batch_n']), noises=[noise[0:2], noise[2:4]])
    lo = lo.cpu().numpy()
    assert abs(lo[0] - g['rec_loss'][0]) <= RTOL * abs(g['rec_loss'][0])
    assert abs(cl.item() - g['cl_loss'][0]) <= RTOL * abs(g['cl_loss'][0])
    E = eng.E0.cpu().numpy()
    assert close(E[:U], g['user_k1']) and close(E[U:], g['item_k1'])
    assert float(eng.G.abs().max()) == 0.0 and int(eng.flags.max()) == 0 and int(eng.dup_bits.abs().max()) == 0


@pytest.mark.parametrize('L,lc', [(1, 1), (3, 1), (3, 2), (3, 3)])
def test_xsimgcl_fused_step_equals_autograd_route_for_other_depths(mods, ml100k, L, lc):
    """step_xsimgcl's schedule (row-subset last hop, masked first backward hop, where G_cl enters the Horner recursion) for depths
    and layer_cl values the reference's hard-coded L=2 / layer_cl=1 golden does not reach, against the encoder's autograd node
    (itself pinned on the golden)."""
    ops, engine = mods
    from types import SimpleNamespace
    from arlib_amd.recommender.XSimGCL import XSimGCL_Encoder
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss, InfoNCE
    import scipy.sparse as sp
    rng = np.random.default_rng(L * 10 + lc)
    U, I, d, B = ml100k['U'], ml100k['I'], 16, 1024
    p0 = ml100k['pairs0']
    half = sp.csr_matrix((np.ones(len(p0), np.float32), (p0[:, 0], p0[:, 1] + U)), shape=(U + I, U + I))
    adj = half + half.T
    dinv = 1.0 / np.sqrt(np.asarray(adj.sum(1)).ravel())
    norm = sp.diags(dinv) @ adj @ sp.diags(dinv)
    enc = XSimGCL_Encoder(SimpleNamespace(user_num=U, item_num=I, norm_adj=norm.tocsr()), d, 0.1, L, lc).cuda()
    E0 = torch.cat([enc.embedding_dict['user_emb'].detach(), enc.embedding_dict['item_emb'].detach()], 0).clone() * 20      # O(0.5) entries
    with torch.no_grad():
        enc.embedding_dict['user_emb'][:] = E0[:U]; enc.embedding_dict['item_emb'][:] = E0[U:]
    noise = [torch.rand(U + I, d, device=DEV) for _ in range(L)]
    sel = rng.integers(0, len(p0), B)
    u, p = T(p0[sel, 0].astype(np.int64)), T(p0[sel, 1].astype(np.int64))
    n = T(rng.integers(0, I, B).astype(np.int64))
    opt = torch.optim.Adam(enc.parameters(), lr=0.005)
    ru, ri, cu, ci = enc(True, noises=noise)
    ui, ii = torch.unique(u), torch.unique(p)
    cl = 0.2 * (InfoNCE(ru[ui], cu[ui], 0.1) + InfoNCE(ri[ii], ci[ii], 0.1))
    loss = bpr_loss(ru[u], ri[p], ri[n]) + l2_reg_loss(1e-4, ru[u], ri[p]) + cl
    opt.zero_grad(); loss.backward(); opt.step()
    ref = torch.cat([enc.embedding_dict['user_emb'], enc.embedding_dict['item_emb']], 0).detach().cpu().numpy()
    eng = engine.PropagationEngine(enc._graph(), U, I, d, L, 1e-4, 0.005, DEV, skip_layer0=True, table=E0.clone())
    lo, cl2 = eng.step_xsimgcl(u.int(), p.int(), n.int(), cl_rate=0.2, tau=0.1, eps=0.1, layer_cl=lc, noises=noise)
    assert abs(cl2.item() - cl.item()) <= RTOL * abs(cl.item())
    assert rel_err(eng.E0.cpu().numpy(), ref) < RTOL
    assert float(eng.G.abs().max()) == 0.0 and int(eng.flags.max()) == 0 and int(eng.dup_bits.abs().max()) == 0


@pytest.mark.parametrize('L', [1, 3])
def test_sgl_fused_step_equals_autograd_route_for_other_depths(mods, ml100k, L):
    """step_sgl (three graphs, sparse-batch schedule) at depths the reference's hard-coded L=2 golden does not reach, against the
    encoder's autograd passes (pinned on the golden at L=2)."""
    ops, engine = mods
    from types import SimpleNamespace
    from arlib_amd.recommender.SGL import SGL_Encoder
    from arlib_amd.util.loss import bpr_loss, l2_reg_loss
    import scipy.sparse as sp
    rng = np.random.default_rng(L)
    U, I, d, B = ml100k['U'], ml100k['I'], 16, 1024
    p0 = ml100k['pairs0']
    R = sp.csr_matrix((np.ones(len(p0), np.float32), (p0[:, 0], p0[:, 1])), shape=(U, I))
    half = sp.csr_matrix((np.ones(len(p0), np.float32), (p0[:, 0], p0[:, 1] + U)), shape=(U + I, U + I))
    adj = half + half.T
    dinv = 1.0 / np.sqrt(np.asarray(adj.sum(1)).ravel())
    data = SimpleNamespace(user_num=U, item_num=I, norm_adj=(sp.diags(dinv) @ adj @ sp.diags(dinv)).tocsr(), interaction_mat=R)
    enc = SGL_Encoder(data, d, 0.1, L, 0.2, 2).cuda()
    E0 = torch.cat([enc.embedding_dict['user_emb'].detach(), enc.embedding_dict['item_emb'].detach()], 0).clone() * 20
    with torch.no_grad():
        enc.embedding_dict['user_emb'][:] = E0[:U]; enc.embedding_dict['item_emb'][:] = E0[U:]
    v1, v2 = enc.graph_reconstruction(), enc.graph_reconstruction()
    sel = rng.integers(0, len(p0), B)
    u, p = T(p0[sel, 0].astype(np.int64)), T(p0[sel, 1].astype(np.int64))
    n = T(rng.integers(0, I, B).astype(np.int64))
    opt = torch.optim.Adam(enc.parameters(), lr=0.005)
    ue, ie = enc()
    cl = 0.2 * enc.cal_cl_loss([u, p], v1, v2)
    loss = bpr_loss(ue[u], ie[p], ie[n]) + l2_reg_loss(1e-4, ue[u], ie[p]) + cl
    opt.zero_grad(); loss.backward(); opt.step()
    ref = torch.cat([enc.embedding_dict['user_emb'], enc.embedding_dict['item_emb']], 0).detach().cpu().numpy()
    eng = engine.PropagationEngine(enc._graph(), U, I, d, L, 1e-4, 0.005, DEV, table=E0.clone())
    lo, cl2 = eng.step_sgl(u.int(), p.int(), n.int(), v1, v2, cl_rate=0.2, tau=0.2)
    assert abs(cl2.item() - cl.item()) <= RTOL * abs(cl.item())
    assert rel_err(eng.E0.cpu().numpy(), ref) < RTOL
    assert float(eng.G.abs().max()) == 0.0 and int(eng.flags.max()) == 0 and int(eng.dup_bits.abs().max()) == 0

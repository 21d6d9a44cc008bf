"""Mult-VAE / Mult-DAE without a GPU: the float64 restatement (tests/multvae_restatement.py) against torch float64 autograd, the composed route of
arlib_amd/multinomial.py and util.loss.multinomial_nll on CPU tensors against the restatement (fp32 and float64; empty, full and weighted rows), the
C entries' declarations and argument checks, and MultVAE's steps on the CPU composed route against the restatement fed the same (rows, keep, eps).

Tolerances.  float64: both sides do the same O(I) sums in float64, 1e-12 relative to the largest value.  fp32: a logit is a d-term dot product
(error ~ d^0.5 * 6e-8 * |q||E|), lse and the gradients carry it through sums of I terms with positive weights p; 2e-5 relative to the largest value
covers d <= 64, I <= 515 with an order of magnitude to spare and is far below any wrong term (a missing correction moves the results by O(1))."""
import contextlib
import ctypes
import io
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import multvae_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 16), (3, 77, 16), (9, 130, 24), (70, 515, 64)]


def rel(a, b):
    a, b = np.asarray(a.detach() if isinstance(a, torch.Tensor) else a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def draw(B, I, d, weighted, seed=0, density=0.05):
    """q, E, pos [B, I] bool with an empty first row and a full last row where B > 2, w [B, I] | None, g."""
    g = torch.Generator().manual_seed(seed + 1000 * B + I + d)
    q, E = torch.randn(B, d, generator=g), torch.randn(I, d, generator=g) / d ** 0.5
    pos = torch.rand(B, I, generator=g) < density
    pos[:, 0] |= ~pos.any(1)                                          # every row has a positive ...
    if B > 2:
        pos[0], pos[-1] = False, True                                 # ... but the first; the last has every item
    w = (0.25 + 2 * torch.rand(B, I, generator=g)) if weighted else None
    return q, E, pos, w, torch.randn(B, generator=g)


def csr(pos, w=None, dtype=torch.float32, device='cpu'):
    """The positives as the op takes them: (rowptr int32, col int32[, val])."""
    rowptr = torch.zeros(pos.shape[0] + 1, dtype=torch.int32)
    rowptr[1:] = pos.sum(1).cumsum(0)
    out = (rowptr, pos.nonzero()[:, 1].to(torch.int32))
    if w is not None:
        out = out + (w[pos].to(dtype),)
    return tuple(t.to(device) for t in out)


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('B,I,d', SHAPES)
def test_restatement_gradients_equal_float64_autograd(B, I, d, weighted):
    q, E, pos, w, g = draw(B, I, d, weighted)
    nll, lse, dq, dE = R.softmax_nll(q, E, pos, w, g)
    q6, E6 = q.double().requires_grad_(), E.double().requires_grad_()
    z = q6 @ E6.t()
    A = pos.double() if w is None else w.double() * pos.double()
    want = -(A * torch.log_softmax(z, 1)).sum(1)                       # the definition: minus the weighted log-probabilities of the positives
    (want * g.double()).sum().backward()
    assert rel(nll, want.detach()) < 1e-12 and rel(lse, torch.logsumexp(z, 1).detach()) < 1e-14
    assert rel(dq, q6.grad) < 1e-12 and rel(dE, E6.grad) < 1e-12
    if B > 2:
        assert float(nll[0]) == 0.0 and float(dq[0].abs().max()) == 0.0


@pytest.mark.parametrize('dtype,tol', [(torch.float32, 2e-5), (torch.float64, 1e-12)], ids=['fp32', 'float64'])
@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('B,I,d', SHAPES)
def test_composed_route_and_autograd_function_on_cpu(B, I, d, weighted, dtype, tol):
    from arlib_amd import multinomial as mn
    from arlib_amd.util.loss import multinomial_nll
    assert multinomial_nll is mn.multinomial_nll
    q, E, pos, w, g = draw(B, I, d, weighted)
    q, E, g = q.to(dtype), E.to(dtype), g.to(dtype)
    w = None if w is None else w.to(dtype)
    want = R.softmax_nll(q, E, pos, w, g)
    P = csr(pos, w, dtype)
    for chunk in (None, 4):                                            # one panel, and panels that cut the batch
        got = mn.multinomial_softmax_composed(q, E, P, g, want_grad=True, chunk=chunk)
        assert all(t.dtype == dtype for t in got)
        for name, a, b in zip(('nll', 'lse', 'dq', 'dE'), got, want):
            assert rel(a, b) <= tol, (name, chunk, rel(a, b))
    fwd, full = mn.multinomial_softmax_composed(q, E, P), mn.multinomial_softmax_composed(q, E, P, g, want_grad=True)
    assert len(fwd) == 2 and torch.equal(fwd[0], full[0]) and torch.equal(fwd[1], full[1])
    assert mn.multinomial_softmax(q, E, P, g, want_grad=True)[2].dtype == dtype        # the dispatcher on the CPU: the composed route
    if B > 2:
        assert float(got[0][0]) == 0.0 and float(got[2][0].abs().max()) == 0.0          # the empty row
    for route in ('auto', 'composed'):
        ql, El = q.clone().requires_grad_(), E.clone().requires_grad_()
        nll = multinomial_nll(ql, El, P, route=route)
        (nll * g).sum().backward()
        assert rel(nll, want[0]) <= tol and rel(ql.grad, want[2]) <= tol and rel(El.grad, want[3]) <= tol
    with pytest.raises(ValueError):
        multinomial_nll(q, E, P, route='kernel')
    with pytest.raises(Exception):
        multinomial_nll(q, E, P, route='fused')                         # the kernel needs device tensors: no quiet fall-back


def test_supported_and_argument_handling():
    from arlib_amd import multinomial as mn, ops
    assert ops.multinomial_softmax is mn.multinomial_softmax and ops.multinomial_nll is mn.multinomial_nll
    lim = (2 ** 31 - 1) // 128
    assert mn.multinomial_softmax_supported(2048, 100_000, 64) and mn.multinomial_softmax_supported(lim, lim, 128, 2 ** 31 - 1)
    for B, I, d, nnz in ((4, 50, 24, 0), (4, 50, 256, 0), (0, 50, 64, 0), (4, 0, 64, 0), (lim + 1, 50, 64, 0), (4, lim + 1, 64, 0), (4, 50, 64, 2 ** 31)):
        assert not mn.multinomial_softmax_supported(B, I, d, nnz)
    # 'auto' takes the kernel only where profiles/multvae_bench.json has it ahead: cfg2's shapes, not ml-1M's
    assert mn.auto_prefers_kernel(2048, 100_000, 64) and mn.auto_prefers_kernel(500, 100_000, 64) and not mn.auto_prefers_kernel(500, 3706, 64)
    q, E, pos, w, g = draw(3, 20, 16, True)
    with pytest.raises(ValueError):
        mn.multinomial_softmax_composed(q, E[:, :8], csr(pos))          # widths differ
    with pytest.raises(ValueError):
        mn.multinomial_softmax_composed(q, E, (csr(pos)[0][:-1], csr(pos)[1]))
    with pytest.raises(ValueError):
        mn.multinomial_softmax_composed(q, E, csr(pos), want_grad=True)  # gradients without the upstream
    with pytest.raises(ValueError):
        mn.multinomial_softmax_composed(q, E, (csr(pos)[0].long(), csr(pos)[1]))


def test_header_declares_and_library_exports_both_entries():
    from arlib_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'arlib_amd.h')).read()
    declared = set(re.findall(r'\b(arl_[a-z0-9_]+)\s*\(', hdr))
    names = {'arl_multinomial_softmax_f32', 'arl_multinomial_softmax_workspace_bytes'}
    assert names <= declared and names <= set(_lib.EXPORTS)
    assert 'nll[b] = n_b lse_b - sum_{i in pos(b)} w_bi z_bi' in hdr
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
    assert _lib.ABI_VERSION == 34 and _lib.lib().arl_abi_version() == 34


def test_c_entry_rejects_before_any_device_work():
    from arlib_amd import _lib
    L = _lib.lib()
    lim = (2 ** 31 - 1) // 128
    ws = L.arl_multinomial_softmax_workspace_bytes
    assert ws(2048, 100_000, 64, 0) > 0 and ws(2048, 100_000, 64, 1) > ws(2048, 100_000, 64, 0) and ws(2048, 100_000, 64, 1) < 2048 * 100_000 * 4 // 4
    assert ws(4, 50, 24, 1) == 0 and ws(0, 50, 64, 1) == 0 and ws(lim + 1, 50, 64, 1) == 0 and ws(4, lim + 1, 64, 0) == 0
    buf = (ctypes.c_float * 64)()                                       # a 16-byte aligned stand-in for every pointer: nothing is launched, nothing read
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    f = L.arl_multinomial_softmax_f32

    def call(q=p, B=4, E=p, I=50, d=64, rowptr=p, col=p, val=None, nnz=10, trowptr=p, tcol=p, tperm=p, g=p, nll=p, lse=p, dq=p, dE=p, wsp=p):
        return f(q, B, E, I, d, rowptr, col, val, nnz, trowptr, tcol, tperm, g, nll, lse, dq, dE, wsp, None)
    for name in ('q', 'E', 'rowptr', 'col', 'nll', 'lse', 'wsp', 'g', 'trowptr', 'tcol'):
        assert call(**{name: None}) == -1, name                         # ARL_E_NULL
    assert call(val=p, tperm=None) == -1                                # weights need the transposed entries' positions
    assert call(d=24) == -2 and call(d=256) == -2                       # ARL_E_DIM
    assert call(B=lim + 1) == -3 and call(I=lim + 1) == -3 and call(nnz=2 ** 31) == -3      # ARL_E_RANGE
    assert call(B=0) == -4 and call(I=0) == -4 and call(nnz=-1) == -4   # ARL_E_ARG
    assert call(q=ctypes.c_void_p(p.value + 4)) == -4                   # a misaligned table


# ------------------------------------------------------------------------------------------------ the model
def synthetic_data(n_users=300, n_items=200, seed=7):
    """A util/synthetic graph as a DataLoader: of every user with six or more items the last one, where its item keeps two training users, is held out."""
    from arlib_amd.util.synthetic import syn_v1_pairs
    from arlib_amd.util.DataLoader import DataLoader
    pairs = syn_v1_pairs(n_users, n_items, mean_deg=12.0, seed=seed)
    count = np.bincount(pairs[:, 1], minlength=n_items)
    last = np.r_[pairs[1:, 0] != pairs[:-1, 0], True]
    deg = np.bincount(pairs[:, 0], minlength=n_users)
    test = last & (deg[pairs[:, 0]] >= 6)
    for k in np.nonzero(test)[0]:
        if count[pairs[k, 1]] > 2:
            count[pairs[k, 1]] -= 1
        else:
            test[k] = False
    tr, te = pairs[~test], pairs[test]
    one = lambda p: (p[:, 0], p[:, 1], np.ones(len(p)))
    return DataLoader.from_arrays(one(tr), None, one(te), dataName='syn', array_native=False)


def rec_args(**kw):
    a = dict(dataset='syn', model_name='MultVAE', maxEpoch=2, batch_size=2048, emb_size=16, n_layers=0, reg=1e-4, lRate=0.01, seed=2018, topK='10',
             vae_batch_users=64, vae_anneal_steps=2, vae_beta=0.5, vae_reg=1e-3)
    a.update(kw)
    return SimpleNamespace(**a)


def fresh(data, **kw):
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender import MultVAE
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        return MultVAE(rec_args(**kw), data)


def batches_for(rec, n_steps, seed=3, with_empty_user=False):
    """n_steps batches (rows, keep, eps) drawn from a generator of the test's own."""
    g = torch.Generator().manual_seed(seed)
    U, B, d = rec.data.user_num, rec.vae_batch_users, rec.model.latent_size
    rp = rec.model.rowptr.cpu()
    out = []
    for _ in range(n_steps):
        rows = torch.randperm(U, generator=g)[:B]
        nnz = int((rp[rows + 1] - rp[rows]).sum())
        out.append((rows, torch.rand(nnz, generator=g) >= rec.vae_dropout, torch.randn(B, d, generator=g)))
    return out


def dense_profiles_of(rec):
    rp, col = rec.model.rowptr.cpu(), rec.model.col.cpu().long()
    X = torch.zeros(rec.data.user_num, rec.data.item_num, dtype=torch.bool)
    X[torch.repeat_interleave(torch.arange(rec.data.user_num), rp[1:] - rp[:-1]), col] = True
    return X


@pytest.fixture(scope='module')
def data():
    return synthetic_data()


@pytest.mark.parametrize('variational', [True, False], ids=['vae', 'dae'])
def test_three_cpu_steps_equal_the_restatement(data, variational):
    rec = fresh(data, vae_variational=variational, vae_route='composed')
    m = rec.model
    d, I = 16, data.item_num
    assert m.embedding_dict['W_enc'].shape == (I, 2 * d if variational else d) and m.embedding_dict['W_dec'].shape == (I, d)
    X = dense_profiles_of(rec)
    assert int(X.sum()) == len(data.training_data) and bool(X.any(1).all())
    W0 = [m.embedding_dict[k].detach().clone() for k in ('W_enc', 'b_enc', 'W_dec')]
    batches = batches_for(rec, 3)
    want, outs = R.train_steps(*W0, X, batches, lr=0.01, vae_beta=0.5, anneal_steps=2, reg=1e-3, dropout=0.5, variational=variational)
    opt = torch.optim.Adam(rec._params(), lr=0.01)
    for t, (rows, keep, eps) in enumerate(batches):
        assert rec.beta() == (R.beta_at(t, 0.5, 2) if variational else 0.0)
        loss, nll, kl = m.step_loss(rows, keep, eps, rec.beta(), rec.vae_reg, rec.vae_dropout, 'composed')
        grads = torch.autograd.grad(loss, rec._params())
        r = outs[t]
        assert abs(float(loss.detach()) - float(r['loss'])) <= 2e-6 * float(r['loss']) and abs(float(nll) - float(r['nll'])) <= 2e-6 * float(r['nll'])
        assert abs(float(kl) - float(r['kl'])) <= 2e-6 * max(float(r['kl']), 1e-3)
        for name, gr, w in zip(('dW_enc', 'db_enc', 'dW_dec'), grads, (r['dW_enc'], r['db_enc'], r['dW_dec'])):
            assert rel(gr, w) <= 2e-5, (t, name, rel(gr, w))
        got = rec.step(rows, keep, eps, opt)
        assert float(got[0]) == float(loss.detach())                            # a pure function of (rows, keep, eps) and the weights
    assert rec.steps_done == 3
    # Adam divides by |g|-sized denominators: an entry moves by about lr per step whatever its gradient, so entries with |g| near 0 may differ in sign
    for p, w in zip(rec._params(), want):
        diff = (p.detach().double() - w).abs()
        assert float((diff < 1e-5).double().mean()) > 0.999 and float(diff.max()) < 0.031


def test_model_shapes_and_guards(data):
    from arlib_amd.recommender import MultVAE
    rec = fresh(data)
    assert isinstance(rec, MultVAE) and (rec.vae_beta, rec.vae_anneal_steps, rec.vae_dropout, rec.vae_batch_users, rec.vae_reg) == (0.5, 2, 0.5, 64, 1e-3)
    args = rec_args()
    for k in ('vae_batch_users', 'vae_anneal_steps', 'vae_beta', 'vae_reg'):
        delattr(args, k)
    with contextlib.redirect_stdout(io.StringIO()):
        plain = MultVAE(args, data)
    assert (plain.vae_beta, plain.vae_anneal_steps, plain.vae_dropout, plain.vae_batch_users, plain.vae_reg, plain.vae_variational, plain.vae_route) == \
        (0.2, 20000, 0.5, 500, 0.0, True, 'auto')
    ue, ie = rec.model()
    assert ue.shape == (data.user_num, 16) and ie.shape == (data.item_num, 16) and ie is rec.model.embedding_dict['W_dec']
    # user_emb is mu of the whole profile: the restatement's encoder without dropout
    X = dense_profiles_of(rec).double()
    W, b = rec.model.embedding_dict['W_enc'].detach().double(), rec.model.embedding_dict['b_enc'].detach().double()
    mu = (X / X.sum(1, keepdim=True).sqrt()) @ W[:, :16] + b[:16]
    assert rel(ue, mu) <= 2e-6
    for kw in (dict(requires_grad=True), dict(requires_embgrad=True), dict(requires_adjgrad=True)):
        with pytest.raises(NotImplementedError):
            rec.train(**kw)
    with pytest.raises(ValueError):
        fresh(data, vae_route='kernel')
    with pytest.raises(ValueError):
        rec.model.step_loss(torch.arange(4), torch.ones(3, dtype=torch.bool), torch.zeros(4, 16), 0.0)

"""GSPAttack on the device: the streaming all-pairs BCE kernel (csrc/arl_allpairs.hip) against the float64 restatement (tests/gsp_restatement.py) at
ragged sizes, its determinism and edge cases, the composed route past its limits, the poisoned hop's gradients, and one whole attack against the
float64 restatement with injected Gumbel noise.  The poisoned-memory runs are in test_gpu_gsp_poison.py."""
import numpy as np
import pytest
import torch
from conftest import close
from test_shilling_cpu import attack_args
import gsp_restatement as rs
import stream_splits_restatement as splits

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def problem(R, I, d, per_row, scale, seed, weighted=False):
    """Tables, per_row distinct positives in every row (sorted), weights in (0, 1.1) when asked, and the ragged row weights of a table three rows
    longer (sliced, as the attack slices the real users' rows)."""
    from arlib_amd import allpairs
    g = torch.Generator().manual_seed(seed)
    Pu, Pi = torch.randn(R, d, generator=g) * scale, torch.randn(I, d, generator=g) * scale
    col = torch.sort(torch.rand(R, I, generator=g).argsort(1)[:, :per_row], 1)[0].reshape(-1).to(torch.int32)
    rowptr = (torch.arange(R + 1) * per_row).to(torch.int32)
    val = (torch.rand(R * per_row, generator=g) * 1.1).clamp_min(1e-3) if weighted else None
    rw = allpairs.batch_mean_row_weights(R + 3, I)[:R].contiguous()
    return Pu, Pi, rowptr, col, val, rw


def on_device(Pu, Pi, rowptr, col, val, rw):
    pos = (rowptr.to(DEV), col.to(DEV)) + ((val.to(DEV),) if val is not None else ())
    return Pu.to(DEV), Pi.to(DEV), pos, rw.to(DEV)


def restated(Pu, Pi, rowptr, col, val, rw, upstream=1.0):
    A = rs.dense_targets(Pu.shape[0], Pi.shape[0], rowptr.numpy(), col.numpy(), None if val is None else val.numpy())
    return rs.bce_allpairs(Pu.numpy(), Pi.numpy(), A, rw.numpy(), upstream=upstream)


# (R, I, d, positives per row, scale): every width; R and I off the 16 / 64-row tiles; R = 1; (9001, 130) and (20000, 70) split the streamed users
# 3 and 5 ways (asserted in the test through splits.USER_SPLIT_COUNTS); scale 0.6 at d = 64 puts scores near +-12, where sigmoid(-|s|) is within two
# orders of eps; (63, 65) has no positives at all; (4097, 65) is the smallest table that splits, 2 x 2049: split 0 ends one row into its 33rd stage
# and the seam is not a multiple of 4
SHAPES = [(1, 37, 16, 3, 0.3), (130, 77, 16, 5, 0.3), (1000, 333, 32, 10, 0.2), (777, 1682, 64, 20, 0.1), (2049, 515, 128, 4, 0.1),
          (9001, 130, 64, 5, 0.15), (20000, 70, 32, 2, 0.2), (257, 130, 64, 6, 0.6), (63, 65, 128, 0, 0.1), (4097, 65, 32, 3, 0.2)]
FACTOR, FLOOR = 4.0, 1e-6
NAMES = ('loss', 'rowloss', 'dPu', 'dPi')


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('R,I,d,per_row,scale', SHAPES)
def test_kernel_against_float64(R, I, d, per_row, scale, weighted):
    """Bar (the one test_gpu_legup.py uses): the composed fp32 torch route's own error against float64 on the same inputs, times FACTOR = 4, with
    FLOOR = 1e-6 where the composed route lands closer than that; max-norm relative error of loss, rowloss, dPu and dPi.  Measured on the MI355X,
    worst case over SHAPES: see DESIGN.md section 3j."""
    from arlib_amd import ops
    assert splits.split_count(I, R)[0] == splits.USER_SPLIT_COUNTS.get((R, I), 1)          # the streamed users' splits this shape is here for
    host = problem(R, I, d, per_row, scale, seed=R + I, weighted=weighted)
    want = restated(*host)
    if scale > 0.5:
        assert float((host[0] @ host[1].t()).abs().max()) > 11.0
    Pu, Pi, pos, rw = on_device(*host)
    got = ops.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True)
    comp = ops.bce_allpairs_loss_composed(Pu, Pi, pos, rw, want_grad=True)
    lo = ops.bce_allpairs_loss(Pu, Pi, pos, rw)
    assert len(lo) == 2 and torch.equal(lo[0], got[0]) and torch.equal(lo[1], got[1])      # the loss-only call gives the same bits
    for name, k, c, w in zip(NAMES, got, comp, want):
        ek, ec = rel(k.cpu().numpy().reshape(np.shape(w)), w), rel(c.cpu().numpy().reshape(np.shape(w)), w)
        print('bce_allpairs R=%d I=%d d=%d nnz/row=%d scale=%g weighted=%d %s: kernel %.3e composed %.3e' % (R, I, d, per_row, scale, weighted, name, ek, ec))
        assert ek <= max(FACTOR * ec, FLOOR), (name, ek, ec)


def test_deterministic():
    from arlib_amd import ops
    Pu, Pi, pos, rw = on_device(*problem(9001, 1300, 64, 7, 0.15, seed=2, weighted=True))
    a = ops.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True)
    b = ops.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    pos_t = ops.transpose_positives(pos[0], pos[1], 9001, 1300)                            # the caller's own by-item form gives the same bits
    for x, y in zip(a, ops.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True, pos_t=pos_t)):
        assert torch.equal(x, y)


def test_repeated_positive_counts_as_listed_and_upstream_scales_exactly():
    from arlib_amd import ops, allpairs
    R, I, d = 300, 200, 32
    g = torch.Generator().manual_seed(5)
    Pu, Pi = torch.randn(R, d, generator=g) * 0.2, torch.randn(I, d, generator=g) * 0.2
    deg = torch.zeros(R, dtype=torch.int64); deg[3] = 3; deg[100] = 2
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32)
    col = torch.tensor([7, 7, 150, 0, 199], dtype=torch.int32)                            # (3, 7) listed twice
    val = torch.tensor([0.5, 0.25, 1.0, 0.75, 1.0])
    rw = allpairs.batch_mean_row_weights(R, I)
    for v in (None, val):
        want = restated(Pu, Pi, rowptr, col, v, rw)
        P = on_device(Pu, Pi, rowptr, col, v, rw)
        got = ops.bce_allpairs_loss(*P, want_grad=True)
        for k, w in zip(got, want):
            assert rel(k.cpu().numpy().reshape(np.shape(w)), w) <= 1e-5
        half = ops.bce_allpairs_loss(*P, want_grad=True, upstream=0.5)
        assert torch.equal(half[0], got[0]) and torch.equal(half[1], got[1])
        assert torch.equal(half[2], 0.5 * got[2]) and torch.equal(half[3], 0.5 * got[3])


def test_empty_rows_next_to_a_full_row():
    from arlib_amd import ops, allpairs
    R, I, d = 70, 150, 64
    g = torch.Generator().manual_seed(8)
    Pu, Pi = torch.randn(R, d, generator=g) * 0.2, torch.randn(I, d, generator=g) * 0.2
    deg = torch.zeros(R, dtype=torch.int64); deg[17] = I; deg[69] = 1
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(torch.int32)
    col = torch.cat([torch.arange(I), torch.tensor([149])]).to(torch.int32)
    rw = allpairs.batch_mean_row_weights(R, I)
    want = restated(Pu, Pi, rowptr, col, None, rw)
    got = ops.bce_allpairs_loss(*on_device(Pu, Pi, rowptr, col, None, rw), want_grad=True)
    for k, w in zip(got, want):
        assert rel(k.cpu().numpy().reshape(np.shape(w)), w) <= 1e-5
    with pytest.raises(IndexError):                                                        # the index arrays are validated before any launch
        ops.bce_allpairs_loss(*on_device(Pu, Pi, rowptr, torch.where(col == 149, 150, col).to(torch.int32), None, rw))


def test_past_the_limits_takes_the_composed_route(monkeypatch):
    from arlib_amd import ops, allpairs as ap
    assert ops.bce_allpairs is ap.bce_allpairs                                             # ops re-exports the module; the limits are the module's
    P = on_device(*problem(500, 300, 64, 5, 0.1, seed=6, weighted=True))
    kern = ops.bce_allpairs(*P, want_grad=True)
    calls = []
    orig = ap.bce_allpairs_loss_composed
    monkeypatch.setattr(ap, 'bce_allpairs_loss_composed', lambda *a, **k: calls.append(1) or orig(*a, **k))
    assert not calls
    monkeypatch.setattr(ap, 'ALLPAIRS_MAX_ROWS', 400)
    assert not ops.bce_allpairs_supported(500, 300, 64, 2500)
    comp = ops.bce_allpairs(*P, want_grad=True)
    assert calls == [1]
    for k, c in zip(kern, comp):
        assert rel(k.cpu().numpy(), c.cpu().numpy()) <= 1e-5
    with pytest.raises(ValueError):
        ops.bce_allpairs_loss(*P)
    monkeypatch.undo()
    host = problem(200, 100, 48, 3, 0.1, seed=8)                                           # a width the kernel does not take
    assert not ops.bce_allpairs_supported(200, 100, 48, 600)
    got = ops.bce_allpairs(*on_device(*host), want_grad=True)
    for k, w in zip(got, restated(*host)):
        assert rel(k.cpu().numpy().reshape(np.shape(w)), w) <= 1e-5


# ------------------------------------------------------------------------------------------------ the poisoned hop
def small_graph(U, I, per_user, seed):
    rng = np.random.default_rng(seed)
    A = np.zeros((U, I), np.float32)
    for u in range(U):
        A[u, rng.choice(I, per_user, replace=False)] = 1
    return A


def test_poisoned_hop_gradients():
    """P = A_hat E with gradients to E and to the fake block S (d^-1/2 held constant): the float64 dense restatement's autograd gradients, themselves
    checked by central differences at a few entries, against the hop Function's, by conftest.close (1e-4)."""
    import scipy.sparse as sp
    from arlib_amd.attack.Black.GSPAttack import poisoned_hop
    from arlib_amd.attack.White.PGA import FactoredFakeGraph
    U, F, I, d = 40, 3, 30, 16
    A = small_graph(U, I, 4, seed=1)
    g = torch.Generator().manual_seed(4)
    E = torch.randn(U + F + I, d, generator=g)
    S = torch.rand(F, I, generator=g) + 0.05
    Wt = torch.randn(U + F + I, d, generator=g)
    A64 = torch.from_numpy(A).double()

    def f64(E64, S64, degrees_from=None):
        P = rs.normalised_adjacency(A64, S64, degrees_from) @ E64
        return (P * Wt.double()).sum(), P

    E64, S64 = E.double().requires_grad_(), S.double().requires_grad_()
    val, P64 = f64(E64, S64)
    dE64, dS64 = torch.autograd.grad(val, (E64, S64))
    h = 1e-6
    for idx in [(0, 0), (2, 17), (1, 29)]:
        Sp, Sm = S.double().clone(), S.double().clone()
        Sp[idx] += h; Sm[idx] -= h
        fd = (f64(E.double(), Sp, S.double())[0] - f64(E.double(), Sm, S.double())[0]) / (2 * h)
        assert abs(float(fd) - float(dS64[idx])) <= 1e-6 * max(1.0, abs(float(fd)))
    for idx in [(0, 0), (41, 5), (60, 15)]:
        Ep, Em = E.double().clone(), E.double().clone()
        Ep[idx] += h; Em[idx] -= h
        fd = (f64(Ep, S.double())[0] - f64(Em, S.double())[0]) / (2 * h)
        assert abs(float(fd) - float(dE64[idx])) <= 1e-6 * max(1.0, abs(float(fd)))
    fg = FactoredFakeGraph(sp.csr_matrix(A), U, F, I, device=DEV, emb_size=d)
    Ed, Sd = E.to(DEV).requires_grad_(), S.to(DEV).requires_grad_()
    fg.set_block(Sd.detach())
    P = poisoned_hop(Ed, Sd, fg)
    (P * Wt.to(DEV)).sum().backward()
    assert close(P.detach().cpu().numpy(), P64.detach().numpy())
    assert close(Ed.grad.cpu().numpy(), dE64.numpy())
    assert close(Sd.grad.cpu().numpy(), dS64.numpy())


# ------------------------------------------------------------------------------------------------ one attack against the float64 restatement
ATTACK_SEED = 2           # chosen on the CPU: the float64 restatement's smallest top-2 gap is 1.9e-2 with this seed


def attack_problem(seed=ATTACK_SEED, U=300, I=120, F=4, k=6, T=2, d=16, epochs=3):
    """A 300 x 120 data set in which every user and item occurs, fp32-representable starting parameters (Xavier-uniform tables and W, torch's
    Linear initialisation for the MLP) and the Gumbel noise of every epoch, all from CPU generators.  Needs no GPU."""
    from arlib_amd.util.DataLoader import DataLoader
    rng = np.random.default_rng(seed)
    pairs = set((u, int(i)) for u in range(U) for i in rng.choice(I, 8, replace=False))
    pairs |= set((int(rng.integers(U)), i) for i in range(I))
    pairs = np.array(sorted(pairs))
    data = DataLoader.from_arrays((pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32)), dataName='gsp-syn', array_native=False)
    assert (data.user_num, data.item_num) == (U, I)
    g = torch.Generator().manual_seed(seed)
    H = int(np.sqrt(I))

    def xavier(r, c):
        b = float(np.sqrt(6.0 / (r + c)))
        return (torch.rand(r, c, generator=g) * 2 - 1) * b

    def uniform(shape, fan_in):
        b = 1.0 / float(np.sqrt(fan_in))
        return (torch.rand(*shape, generator=g) * 2 - 1) * b
    params = dict(user_emb=xavier(U + F, d), item_emb=xavier(I, d), w1=[xavier(d, d) for _ in range(2)], w2=[xavier(d, d) for _ in range(2)],
                  mlp_w0=uniform((H, 2 * d), 2 * d), mlp_b0=uniform((H,), 2 * d), mlp_w1=uniform((1, H), H), mlp_b1=uniform((1,), H))
    noises = [-torch.empty(k, F, I).exponential_(generator=g).log() for _ in range(epochs)]
    args = attack_args('GSPAttack', 'Black', maliciousUserSize=F, maliciousFeedbackSize=k, targetSize=T, Epoch=epochs)
    return data, args, params, noises


def restated_attack(interact, targets, k, params, noises):
    p64 = {n: ([w.double().requires_grad_() for w in v] if isinstance(v, list) else v.double().requires_grad_()) for n, v in params.items()}
    A_real = torch.from_numpy((np.asarray(interact.todense()) != 0).astype(np.float64))
    return rs.run_attack(p64, A_real, list(targets), int(k), [n.double() for n in noises])


def load_parameters(ngcf, params):
    with torch.no_grad():
        ngcf.embedding_dict['user_emb'].copy_(params['user_emb']); ngcf.embedding_dict['item_emb'].copy_(params['item_emb'])
        for i in range(len(params['w1'])):
            ngcf.W['w1_%d' % i].copy_(params['w1'][i]); ngcf.W['w2_%d' % i].copy_(params['w2'][i])
        ngcf.mlp.net[0].weight.copy_(params['mlp_w0']); ngcf.mlp.net[0].bias.copy_(params['mlp_b0'])
        ngcf.mlp.net[2].weight.copy_(params['mlp_w1']); ngcf.mlp.net[2].bias.copy_(params['mlp_b1'])


def run_device_attack(data, args, params, noises):
    import random
    from arlib_amd.attack.Black.GSPAttack import GSPAttack
    random.seed(7)
    atk = GSPAttack(args, data, emb_size=params['user_emb'].shape[1])
    before = atk.interact.copy()
    atk.ngcf = atk._proxy()
    load_parameters(atk.ngcf, params)
    it = iter(noises)
    atk._noise = lambda shape: next(it).to(DEV)
    res = atk.posionDataAttack()
    return atk, before, res


def test_one_attack_against_float64():
    data, args, params, noises = attack_problem()
    atk, before, res = run_device_attack(data, args, params, noises)
    want = restated_attack(before, atk.targetItem, atk.maliciousFeedbackNum, params, noises)
    U, F, I, k, T = 300, 4, 120, 6, 2
    print('gsp attack: smallest top-2 gap %.3e, losses %s (float64 %s)' % (want['gap'], atk.loss_log, want['loss']))
    assert want['gap'] >= 1e-3                                                             # no fp32 / fp64 near-tie can flip a pick
    assert len(atk.pick_log) == 3 and all(torch.equal(a, b) for a, b in zip(atk.pick_log, want['picks']))
    assert len(atk.loss_log) == 3 and close(np.asarray(atk.loss_log), np.asarray(want['loss']))
    assert close(atk.first_dS.cpu().numpy(), want['dS'].numpy())
    assert res.shape == (U + F, I) == atk.interact.shape and (res[:U] != before).nnz == 0
    fake = np.asarray(res[U:].todense())
    assert set(np.unique(fake).tolist()) <= {0.0, 1.0}
    assert (fake[:, atk.targetItem] == 1).all() and ((fake.sum(1) >= k) & (fake.sum(1) <= k + T)).all()
    assert atk.fakeUser == list(range(U, U + F))

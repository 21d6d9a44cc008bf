"""GOAT on the device: the co-rating degree kernel (csrc/arl_corating.hip) against the numpy expression at the bitmap's word edges, with a hub, an
empty column, lone users and at the full LDS size; one D and one G step against a float64 restatement; the short and the long training run against
the reference's (g32, tests/golden/gen_golden_goat.py); reuse, pickling, dataSave and the attack in the ARLib flow."""
import contextlib
import copy
import hashlib
import io
import os
import pickle
import random
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as Fn
from conftest import golden
from test_host_api import make_data
from test_shilling_cpu import attack_args, block

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def reseed(seed=11):
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)


def state_shas():
    st = np.random.get_state()
    return dict(random_state_sha=sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8)),
                numpy_state_sha=sha(np.asarray(st[1], np.uint32), np.asarray([st[2]], np.int64)), torch_state_sha=sha(torch.get_rng_state().numpy()))


# ---------------------------------------------------------------------------------------------------- co-rating degree
def numpy_degree(D):
    D = np.asarray(D, np.float64)
    return ((D.T @ D) > 0).sum(0).astype(np.int64)


def device_degree(X):
    from arlib_amd import corating
    X = sp.csr_matrix(X)
    out = corating.corating_degree(X.indptr, X.indices, X.shape[0], X.shape[1])
    assert out.dtype == torch.int32 and out.is_cuda and out.shape == (X.shape[1],)
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize('I', [1, 31, 32, 33, 64, 65])
def test_degree_at_the_bitmap_word_edges(I):
    rng = np.random.RandomState(I)
    D = (rng.random_sample((7, I)) < 0.3).astype(np.float32)
    D[3, I - 1] = 1                                                  # the last bit of the last word is set by someone
    assert np.array_equal(device_degree(D), numpy_degree(D))
    assert np.array_equal(device_degree(np.ones((7, I))), np.full(I, I))         # every bit of every word


def test_degree_on_ml100k():
    g = golden('g32_goat.npz')
    X = sp.csr_matrix(make_data().matrix())
    got = device_degree(X)
    assert got.shape == (1412,) and np.array_equal(got.astype(np.float64), g['item_int_num'])


def hub_problem():
    """U 300 x I 4 099 (a ragged last word): item 7 rated by every user (the hub), item 11 by nobody, user 5 without items, user 6 with item 4098
    only (a count of 1, in the last word), user 8 with the hub only."""
    rng = np.random.RandomState(5)
    D = (rng.random_sample((300, 4099)) < 0.004).astype(np.float32)
    D[:, 4098] = 0
    D[:, 7] = 1
    D[:, 11] = 0
    D[5] = 0
    D[6] = 0; D[6, 4098] = 1
    D[8] = 0; D[8, 7] = 1
    return sp.csr_matrix(D)


def test_degree_with_a_hub_an_empty_column_and_lone_users():
    from arlib_amd import corating
    X = hub_problem()
    got = device_degree(X)
    want = corating.corating_degree_host(X).astype(np.int64)
    assert np.array_equal(want, np.asarray(((X.T @ X) > 0).sum(0)).ravel())
    assert np.array_equal(got, want)
    assert got[11] == 0 and got[4098] == 1 and got[7] == np.count_nonzero(np.asarray(X.sum(0)).ravel()) - 1      # the hub meets every rated item but 4098, whose only user lacks it
    # stored order within a row and repeated entries do not matter
    rp, col = X.indptr, X.indices.copy()
    for u in range(300):
        col[rp[u]:rp[u + 1]] = col[rp[u]:rp[u + 1]][::-1]
    assert np.array_equal(corating.corating_degree(rp, col, 300, 4099).cpu().numpy(), want)
    rp2, col2 = np.concatenate([rp, [rp[-1] + 3]]), np.concatenate([col, [4098, 7, 7]])          # one more user: {7, 4098}, the hub listed twice
    want2 = corating.corating_degree_host(sp.csr_matrix((np.ones(len(col2)), col2, rp2), shape=(301, 4099))).astype(np.int64)
    assert want2[4098] == 2 and want2[7] == want[7] + 1
    assert np.array_equal(corating.corating_degree(rp2, col2, 301, 4099).cpu().numpy(), want2)


def test_degree_is_identical_from_call_to_call():
    from arlib_amd import corating
    X = hub_problem()
    a = corating.corating_degree(X.indptr, X.indices, 300, 4099)
    b = corating.corating_degree(X.indptr, X.indices, 300, 4099)
    assert torch.equal(a, b)


def test_degree_at_the_full_lds_size():
    """I = CORATING_MAX_ITEMS with two users: the launch takes all 160 KiB of LDS; items of the first word, of the last word and in between."""
    from arlib_amd import corating
    I = corating.CORATING_MAX_ITEMS
    rng = np.random.RandomState(9)
    a = np.unique(np.concatenate([[0, 1, 31, I - 1], rng.randint(0, I, 700)]))
    b = np.unique(np.concatenate([[1, 32, I - 33, I - 2], rng.randint(0, I, 500)]))
    rp, col = np.array([0, len(a), len(a) + len(b)], np.int64), np.concatenate([a, b]).astype(np.int32)
    got = corating.corating_degree(rp, col, 2, I).cpu().numpy()
    in_a, in_b = np.zeros(I, bool), np.zeros(I, bool)
    in_a[a], in_b[b] = True, True
    both = len(np.union1d(a, b))
    want = np.where(in_a & in_b, both, np.where(in_a, len(a), np.where(in_b, len(b), 0)))
    assert np.array_equal(got, want) and got[1] == both and got[I - 1] == len(a) and got[I - 2] == len(b)


def test_one_item_past_the_limit_takes_the_host_route(monkeypatch):
    from arlib_amd import corating
    from arlib_amd.attack.Gray.GOAT import GOAT
    I = corating.CORATING_MAX_ITEMS + 1
    assert not corating.corating_degree_supported(I) and corating.corating_degree_supported(I - 1)
    X = sp.csr_matrix((np.ones(5, np.float32), (np.array([0, 0, 1, 1, 1]), np.array([0, I - 1, 0, 5, 77]))), shape=(2, I))
    with pytest.raises(ValueError, match='corating_degree_host'):
        corating.corating_degree(X.indptr, X.indices, 2, I)

    def never(*a, **k):
        raise AssertionError('the kernel route was taken')
    monkeypatch.setattr(corating, 'corating_degree', never)
    got = GOAT.co_rating(X)
    assert got.dtype == np.float64 and got[0] == 4 and got[I - 1] == 2 and got[5] == got[77] == 3 and got.sum() == 4 + 2 + 3 + 3


# ---------------------------------------------------------------------------------------------------- float64 restatement
def named(G, D):
    return dict([('G.' + n, p) for n, p in G.named_parameters()] + [('D.' + n, p) for n, p in D.named_parameters()])


def f64_G(P, Z, k):
    lrelu = lambda x: Fn.leaky_relu(x, 0.2)

    def mlp(x, pre, n):
        for i in range(n):
            x = lrelu(Fn.linear(x, P['%s.net.layer_%d.weight' % (pre, i)], P['%s.net.layer_%d.bias' % (pre, i)]))
        return x
    L_t = mlp(Z, 'G.G_l', 3)
    H = mlp(Z, 'G.G_e', 3).reshape(Z.shape[0], k, 16)
    R = (H @ (L_t.T @ L_t)).reshape(Z.shape[0], 16 * k)
    return mlp(R, 'G.G_r', 1)


def f64_D(P, x):
    for i in range(4):
        x = torch.sigmoid(Fn.linear(x, P['D.D_r.net.layer_%d.weight' % i], P['D.D_r.net.layer_%d.bias' % i]))
    return x


def f64_losses(P, Z, real, k):
    """(loss1, loss2) of the reference's two steps at the parameters P (a dict of float64 tensors)."""
    Y = f64_G(P, Z, k)
    loss1 = (f64_D(P, Y.detach()) - f64_D(P, real)).mean()
    loss2 = (-f64_D(P, Y) + 0.01 * (1 / k) * torch.linalg.norm(Y - real)).mean()
    return loss1, loss2


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


@pytest.fixture(scope='module')
def first_step():
    """g32's starting point: the initial parameters (seed 11: checked against their digests on the CPU), the first captured sample and the first Z."""
    from arlib_amd.attack.Gray.GOAT import Encoder, Decoder
    g = golden('g32_goat.npz')
    torch.manual_seed(int(g['seed']))
    G, D = Encoder(46), Decoder(46)
    Z = torch.randn(9, 46)
    assert sha(Z.numpy()) == str(g['short_z_sha'][0])
    for n, p in named(G, D).items():
        assert sha(p.detach().numpy()) == str(g['init_sha__' + n]), n
    return g, G, D, Z, torch.from_numpy(g['samp46_real'][0].astype(np.float32))


def test_one_d_and_one_g_step_against_float64(first_step):
    """Loss and every parameter gradient of both steps: the device's relative error against float64 is at most twice the CPU fp32 evaluation's of
    the same expressions (or 1e-6), and at most 1e-4.  The CPU side is the reference's expressions in plain fp32 torch.  Its own errors on this
    step: loss1 1.9e-5, D.D_r.net.layer_2.bias 7.7e-5, D.D_r.net.layer_3.bias 1.5e-4 (a difference of two means of sigmoid derivatives near 0.25,
    half an ulp of which is 1.5e-8), every G gradient <= 4.1e-7.  GOAT.d_loss evaluates D in float64 for that reason: device errors <= 4.5e-8 on
    D's side, <= 2.5e-7 on G's."""
    from arlib_amd.attack.Gray import GOAT as M
    g, G, D, Z, real = first_step
    P = {n: p.detach().double().requires_grad_(True) for n, p in named(G, D).items()}
    l1, l2 = f64_losses(P, Z.double(), real.double(), 46)
    dn, gn = [n for n in P if n.startswith('D.')], [n for n in P if n.startswith('G.')]
    ref = dict(loss1=l1.detach(), loss2=l2.detach())
    ref.update(zip(dn, torch.autograd.grad(l1, [P[n] for n in dn])))
    ref.update(zip(gn, torch.autograd.grad(l2, [P[n] for n in gn])))

    def fp32(dev, d_loss, g_loss):
        Gd, Dd = copy.deepcopy(G).to(dev), copy.deepcopy(D).to(dev)
        Pd = named(Gd, Dd)
        a = d_loss(Gd, Dd, Z.to(dev), real.to(dev))
        b = g_loss(Gd, Dd, Z.to(dev), real.to(dev), 46)
        out = dict(loss1=a.detach(), loss2=b.detach())
        out.update(zip(dn, torch.autograd.grad(a, [Pd[n] for n in dn])))
        out.update(zip(gn, torch.autograd.grad(b, [Pd[n] for n in gn])))
        return out

    def plain_d(Gd, Dd, z, r):                       # the reference's expressions in plain fp32 torch
        return (Dd(Gd(z).detach()) - Dd(r)).mean()

    def plain_g(Gd, Dd, z, r, k):
        y = Gd(z)
        return (-Dd(y) + 0.01 * (1 / k) * torch.linalg.norm(y - r)).mean()
    dev, cpu = fp32(DEV, M.d_loss, M.g_loss), fp32('cpu', plain_d, plain_g)
    assert all(v.is_cuda for v in dev.values())
    rows = [(n, rel(dev[n], ref[n]), rel(cpu[n], ref[n])) for n in ref]
    for n, e_dev, e_cpu in rows:
        print('%-32s device %.3e  cpu fp32 %.3e' % (n, e_dev, e_cpu))
    bad = [(n, e_dev, e_cpu) for n, e_dev, e_cpu in rows if not (e_dev <= max(2 * e_cpu, 1e-6) and e_dev <= 1e-4)]
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- the runs against g32
def goat(**kw):
    from arlib_amd.util.tool import seedSet
    from arlib_amd.attack.Gray.GOAT import GOAT
    seedSet(2018)
    return GOAT(attack_args('GOAT', 'Gray', **kw), make_data())


def run(be, e1, e2):
    from arlib_amd.attack.Gray import GOAT as M
    atk = goat()
    atk.BiLevelOptimizationEpoch = be
    zs, orig = [], M.Encoder.forward

    def fwd(self, x):
        zs.append(sha(x.detach().cpu().numpy()))
        return orig(self, x)
    M.Encoder.forward = fwd
    try:
        reseed()
        res = atk.posionDataAttack(epoch1=e1, epoch2=e2)
    finally:
        M.Encoder.forward = orig
    return atk, res, zs, state_shas()


def f64_short_run(g):
    """The short run (2 x (3 D steps + 2 G steps)) restated in float64 on the CPU: the reference's draws, float64 parameters, torch's own Adam."""
    from arlib_amd.attack.Gray import GOAT as M
    X = sp.csr_matrix(make_data().matrix())
    X.sort_indices()
    U, I = X.shape
    reseed()
    G, D = M.Encoder(46), M.Decoder(46)
    P = {n: p.detach().double().requires_grad_(True) for n, p in named(G, D).items()}
    dn, gn = [P[n] for n in P if n.startswith('D.')], [P[n] for n in P if n.startswith('G.')]
    opt_G, opt_D = torch.optim.Adam(gn, lr=0.005), torch.optim.Adam(dn, lr=0.005)
    loss1, loss2 = [], []
    for i in range(2):
        for phase, n in ((0, 3), (1, 2)):
            for _ in range(n):
                real = torch.from_numpy(M.item_sample(X.indptr, X.indices, U, I, g['item_int_num'], g['targets'], 9, 46, 0.01, 0.02)[2].astype(np.float64))
                Z = torch.randn(9, 46).double()
                l1, l2 = f64_losses(P, Z, real, 46)
                opt, params, loss, log = (opt_D, dn, l1, loss1) if phase == 0 else (opt_G, gn, l2, loss2)
                for p, gr in zip(params, torch.autograd.grad(loss, params)):
                    p.grad = gr
                opt.step()
                log.append(float(loss.detach()))
    return np.array(loss1), np.array(loss2)


@pytest.fixture(scope='module')
def short_run():
    g = golden('g32_goat.npz')
    return (g,) + run(2, 3, 2) + (f64_short_run(g),)


def test_short_run_draws_what_the_reference_draws(short_run):
    g, atk, res, zs, shas, _ = short_run
    assert atk.targetItem == g['targets'].tolist() and atk.k == 46 and atk.fakeUserNum == 9
    assert np.array_equal(np.asarray(atk.itemIntNum), g['item_int_num']) and isinstance(atk.itemIntNum[0], float)
    assert zs == g['short_z_sha'].tolist()
    for key, val in shas.items():
        assert val == str(g['short_' + key]), key
    assert res.shape == (atk.userNum + 9, atk.itemNum) and (res.tocsr()[atk.userNum:].getnnz(1) == 46).all()


def test_short_run_losses_within_the_reference_own_spread(short_run):
    """loss1 of the 6 D steps and loss2 of the 4 G steps against the reference's fp32 run.  Bar, per series: 4 x the larger of the reference's own
    1-thread / 4-thread spread and the deviation of the reference's fp32 losses from the float64 restatement of the same ten steps.
    Measured when this was written: spread 6.0e-8 (loss1) / 0 (loss2); reference against float64 4.2e-8 / 5.6e-8; the device run against the
    reference 4.2e-8 / 6.0e-8 (bars 2.4e-7 / 2.2e-7)."""
    g, atk, res, zs, shas, (f1, f2) = short_run
    got = torch.stack(atk.loss_log).double().cpu().numpy()
    got1, got2 = np.concatenate([got[0:3], got[5:8]]), np.concatenate([got[3:5], got[8:10]])
    for name, mine, f64 in (('loss1', got1, f1), ('loss2', got2, f2)):
        ref, ref1 = g['short_' + name], g['short_' + name + '_t1']
        spread, dev64 = np.abs(ref - ref1).max(), np.abs(ref - f64).max()
        diff = np.abs(mine - ref).max()
        print('%s: spread %.3e, reference against float64 %.3e, device against reference %.3e' % (name, spread, dev64, diff))
        assert dev64 < 1e-5                                                # the restatement follows the reference (same draws, same steps)
        assert diff <= 4 * max(spread, dev64), (name, diff, spread, dev64)


def test_short_run_end_parameters(short_run):
    """Every parameter of G and D after the ten steps against the reference's.  Bar per tensor, the one test_gpu_legup.py and test_gpu_aush.py hold
    trained parameters to: 100 x the reference's own spread between four torch threads and one, plus the project's fp32 parity bar of 1e-4 of the
    tensor's largest entry (Adam's normalised step turns last-bit differences of near-zero gradients into moves of up to lr = 5e-3 per step, so
    ten steps of a faithful run can differ by more than rounding; the spread term follows the tensors where the reference shows that itself)."""
    g, atk, res, zs, shas, _ = short_run
    P = named(atk.G, atk.D)
    assert sorted('short_final__' + n for n in P) == sorted(k for k in g.files if k.startswith('short_final__'))
    worst = ('', 0.0)
    for n, p in P.items():
        ref, ref1 = g['short_final__' + n].astype(np.float64), g['short_final_t1__' + n].astype(np.float64)
        bar = 100 * np.abs(ref - ref1).max() + 1e-4 * np.abs(ref).max()
        diff = np.abs(p.detach().cpu().numpy().astype(np.float64) - ref).max()
        worst = max(worst, (n, diff / bar), key=lambda t: t[1])
        assert diff <= bar, (n, diff, bar)
    print('end parameters: largest share of the bar %.3f (%s)' % (worst[1], worst[0]))


@pytest.fixture(scope='module')
def long_run():
    return (golden('g32_goat.npz'),) + run(10, 20, 20)


def test_long_run_fake_block(long_run):
    """The final sample is the reference's; rows whose cut margin exceeds 10 x max |Y - final_Y| have the reference's items exactly (at most 2 of
    the 9 rows may fall below that), the others keep all targets and differ in at most one item."""
    g, atk, res, zs, shas = long_run
    assert np.array_equal(atk.last_sample[0], g['final_Is']) and np.array_equal(atk.last_sample[1], g['final_If'])
    for key, val in shas.items():
        assert val == str(g['long_' + key]), key
    diff = float(np.abs(atk.last_Y.double().cpu().numpy() - g['final_Y']).max())
    print('max |Y - final_Y| = %.3e; cut margins %s' % (diff, g['cut_margin'].tolist()))
    assert (g['targets_kept'] == 5).all() and (g['final_Y'] > 0).all()
    r, c, v = block(res, atk.userNum)
    assert (v == 1).all()
    decided = g['cut_margin'] > 10 * diff
    assert (~decided).sum() <= 2, (diff, g['cut_margin'].tolist())
    for f in range(9):
        mine, ref = set(c[r == f].tolist()), set(g['col'][g['row'] == f].tolist())
        assert len(mine) == 46 and set(atk.targetItem) <= mine
        if decided[f]:
            assert mine == ref, (f, sorted(mine ^ ref))
        else:
            assert len(mine - ref) <= 1, (f, sorted(mine ^ ref))


# ---------------------------------------------------------------------------------------------------- further behaviour
def test_second_call_reuses_the_generator_and_samples_again(long_run):
    g, atk, res, zs, shas = long_run
    W = atk.G.G_r.net.layer_0.weight.detach().clone()
    n, calls = len(atk.loss_log), len(atk.real_users)
    res2 = atk.posionDataAttack(epoch1=20, epoch2=20)
    assert len(atk.loss_log) == n and len(atk.real_users) == calls + 1 and torch.equal(W, atk.G.G_r.net.layer_0.weight)
    assert res2.shape == res.shape and (res2.tocsr()[atk.userNum:].getnnz(1) == 46).all()
    assert (res2.tocsr()[:atk.userNum] != sp.csr_matrix(atk.interact)).nnz == 0
    assert atk.t.shape == (9, atk.itemNum) and np.array_equal(atk.t.to_dense().numpy(), res2.tocsr()[atk.userNum:].toarray())


def test_attack_pickles_and_deep_copies_after_training(long_run):
    g, atk, res, zs, shas = long_run
    for twin in (pickle.loads(pickle.dumps(atk)), copy.deepcopy(atk)):
        assert all(torch.equal(a, b) for a, b in zip(twin.G.parameters(), atk.G.parameters()))
        assert all(torch.equal(a, b) for a, b in zip(twin.D.parameters(), atk.D.parameters()))
        assert twin.itemIntNum == atk.itemIntNum and twin.targetItem == atk.targetItem and twin.D_r is None
        st = random.getstate(), torch.get_rng_state()
        a = atk.posionDataAttack()
        random.setstate(st[0]); torch.set_rng_state(st[1])
        b = twin.posionDataAttack()
        assert (a != b).nnz == 0


def test_flow_with_lightgcn_datasave_and_attack_metric(tmp_path, monkeypatch):
    from test_gpu_random_flow import rec_args
    from arlib_amd.util.tool import seedSet, dataSave
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.FileIO import FileIO
    from arlib_amd.util.metrics import AttackMetric
    from arlib_amd.recommender.LightGCN import LightGCN
    from arlib_amd.attack.Gray.GOAT import GOAT
    monkeypatch.chdir(tmp_path)
    seedSet(2018)
    data = make_data()
    rec = LightGCN(rec_args(), data)
    atk = GOAT(SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular',
                               targetSize=5), data)
    assert atk.recommenderModelRequired is False and atk.recommenderGradientRequired is False and atk.attackForm == 'dataAttack'
    assert atk.BiLevelOptimizationEpoch == 50 and atk.G is None and atk.D_r is None
    atk.BiLevelOptimizationEpoch = 1
    poison = sp.csr_matrix(atk.posionDataAttack(epoch1=2, epoch2=2))
    U, F = data.user_num, atk.fakeUserNum
    assert poison.shape == (U + F, data.item_num) and (poison[:U] != sp.csr_matrix(data.matrix())).nnz == 0
    assert (poison[U:].getnnz(1) == atk.maliciousFeedbackNum).all() and len(atk.loss_log) == 4
    out_dir = 'data/poison/GOAT_ml-100k/0/'
    os.makedirs(out_dir, exist_ok=True)
    dataSave(poison, out_dir + 'train.txt', data.id2user, data.id2item)
    g = golden('ml100k_data.npz')
    for name in ('val', 'test'):
        FileIO.write_file(out_dir, name + '.txt', ['%d %d %s\n' % (a, b, c) for a, b, c in zip(g[name + '_u'].tolist(), g[name + '_i'].tolist(), g[name + '_r'].tolist())])
    pargs = rec_args(dataset='GOAT_ml-100k/0', data_path='data/poison/', training_data='/train.txt', val_data='/val.txt', test_data='/test.txt')
    pdata = DataLoader(pargs)
    assert pdata.user_num == U + F and pdata.item_num == data.item_num and sp.csr_matrix(pdata.matrix()).nnz == poison.nnz
    back = sp.csr_matrix(pdata.matrix())
    pu = [pdata.user[str(data.id2user[u]) if u in data.id2user else 'fakeUser%d' % u] for u in range(U + F)]
    pi = [pdata.item[str(data.id2item[i])] for i in range(data.item_num)]
    assert (back[pu][:, pi] != poison).nnz == 0                              # the round trip keeps every entry, the fake rows included
    rec.__init__(pargs, pdata)
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train()
        _, after = rec.test()
    assert after[0] == 'Top 10\n'
    hr = AttackMetric(rec, atk.targetItem, [10, 50]).hitRate()
    assert len(hr) == 2 and all(0.0 <= x <= 1.0 for x in hr) and hr[0] <= hr[1] + 1e-12

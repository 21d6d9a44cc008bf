"""LegUP on the device: the streaming ranking-loss kernel (csrc/arl_colsoftmax.hip) against the float64 restatement at ragged sizes, its
determinism, the composed route past its limits, the whole attack against the reference's run (g31,
tests/golden/gen_golden_legup.py) and the op at cfg2's shape.  The poisoned-memory runs are in test_gpu_legup_poison.py."""
import random

import numpy as np
import pytest
import torch
from conftest import golden
from test_host_api import make_data
from test_shilling_cpu import attack_args, reseed, block, sha
from legup_restatement import colsoftmax_target_loss as restated
import stream_splits_restatement as splits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PARAMS = ('G.net.layer_0.weight', 'G.net.layer_0.bias', 'G.net.layer_1.weight', 'G.net.layer_1.bias', 'D.net.0.weight', 'D.net.0.bias')


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def problem(U, I, d, T, scale, seed):
    g = torch.Generator().manual_seed(seed)
    Pu, Pi = torch.randn(U, d, generator=g) * scale, torch.randn(I, d, generator=g) * scale
    cols = torch.randperm(I, generator=g)[:T].tolist()
    return Pu.to(DEV), Pi.to(DEV), cols


# every width; U and I off the 16 / 64-row tiles; T = 1 and 5; U = 1; (9001, 130) and (20000, 70) split the streamed users 3 and 5 ways (asserted in
# the test through splits.USER_SPLIT_COUNTS); scale 1.5 at d = 64 puts scores past 88.7, where a plain fp32 exp is inf and only the running maximum
# keeps the sums finite; (4097, 65) is the smallest table that splits, 2 x 2049: split 0 ends one row into its 33rd stage and the seam is not a
# multiple of 4
SHAPES = [(1, 37, 16, 1, 0.3), (130, 77, 16, 5, 0.3), (1000, 333, 32, 5, 0.2), (777, 1682, 64, 5, 0.1), (2049, 515, 128, 1, 0.1),
          (9001, 130, 64, 5, 0.15), (20000, 70, 32, 1, 0.2), (1500, 900, 64, 5, 1.5), (63, 65, 128, 5, 0.1), (4097, 65, 32, 5, 0.2)]
FACTOR, FLOOR = 4.0, 1e-6


@pytest.mark.parametrize('U,I,d,T,scale', SHAPES)
def test_kernel_against_float64(U, I, d, T, scale):
    """Bar: the composed fp32 torch route's own error against float64 on the same inputs, times FACTOR = 4, with FLOOR = 1e-6 (16 fp32 ulps) where
    the composed route happens to land closer than that.  Measured on the MI355X (max-norm relative error, kernel / composed), worst case over SHAPES:
    see DESIGN.md section 3f."""
    from arlib_amd import ops
    assert splits.split_count(I, U)[0] == splits.USER_SPLIT_COUNTS.get((U, I), 1)      # the streamed users' splits this shape is here for
    Pu, Pi, cols = problem(U, I, d, T, scale, seed=U + I)
    want = restated(Pu.cpu().numpy(), Pi.cpu().numpy(), cols, want_grad=True)
    if scale > 1:
        assert float((Pu @ Pi.t()).max()) > 88.8
    got = ops.colsoftmax_target_loss(Pu, Pi, cols, want_grad=True)
    comp = ops.colsoftmax_target_loss_composed(Pu, Pi, cols, want_grad=True)
    lo = ops.colsoftmax_target_loss(Pu, Pi, cols)
    assert torch.equal(lo[0], got[0]) and torch.equal(lo[1], got[1])                   # the loss-only call gives the same bits
    for name, k, c, w in zip(('loss', 'lse', 'dPu', 'dPi'), got, comp, want):
        ek, ec = rel(k.cpu().numpy().reshape(np.shape(w)), w), rel(c.cpu().numpy().reshape(np.shape(w)), w)
        print('colsoftmax U=%d I=%d d=%d T=%d scale=%g %s: kernel %.3e composed %.3e' % (U, I, d, T, scale, name, ek, ec))
        assert ek <= max(FACTOR * ec, FLOOR), (name, ek, ec)


def test_repeated_targets_count_as_listed():
    from arlib_amd import ops
    Pu, Pi, _ = problem(300, 200, 32, 1, 0.2, seed=5)
    cols = [7, 7, 150]
    want = restated(Pu.cpu().numpy(), Pi.cpu().numpy(), cols, want_grad=True)
    got = ops.colsoftmax_target_loss(Pu, Pi, cols, want_grad=True)
    for k, w in zip(got, want):
        assert rel(k.cpu().numpy().reshape(np.shape(w)), w) <= 1e-5


def test_deterministic():
    from arlib_amd import ops
    Pu, Pi, cols = problem(9001, 1300, 64, 5, 0.15, seed=2)
    a = ops.colsoftmax_target_loss(Pu, Pi, cols, want_grad=True)
    b = ops.colsoftmax_target_loss(Pu, Pi, cols, want_grad=True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_past_the_limits_takes_the_composed_route(monkeypatch):
    from arlib_amd import ops, colsoftmax as cs
    assert ops.colsoftmax_target is cs.colsoftmax_target                               # ops re-exports the module; the limits are the module's
    Pu, Pi, cols = problem(500, 300, 64, 5, 0.1, seed=6)
    kern = ops.colsoftmax_target(Pu, Pi, cols, want_grad=True)
    calls = []
    orig = cs.colsoftmax_target_loss_composed
    monkeypatch.setattr(cs, 'colsoftmax_target_loss_composed', lambda *a, **k: calls.append(1) or orig(*a, **k))
    assert not calls
    monkeypatch.setattr(cs, 'COLSOFTMAX_MAX_ROWS', 400)
    assert not ops.colsoftmax_target_supported(500, 300, 64, 5)
    comp = ops.colsoftmax_target(Pu, Pi, cols, want_grad=True)
    assert calls == [1]
    for k, c in zip(kern, comp):
        assert rel(k.cpu().numpy(), c.cpu().numpy()) <= 1e-5
    with pytest.raises(ValueError):
        ops.colsoftmax_target_loss(Pu, Pi, cols)
    monkeypatch.undo()
    Pu48, Pi48, cols = problem(200, 100, 48, 3, 0.1, seed=8)                           # a width the kernel does not take
    assert not ops.colsoftmax_target_supported(200, 100, 48, 3)
    got = ops.colsoftmax_target(Pu48, Pi48, cols, want_grad=True)
    want = restated(Pu48.cpu().numpy(), Pi48.cpu().numpy(), cols, want_grad=True)
    for k, w in zip(got, want):
        assert rel(k.cpu().numpy().reshape(np.shape(w)), w) <= 1e-5
    with pytest.raises(IndexError):
        ops.colsoftmax_target(Pu, Pi, [300])


# ------------------------------------------------------------------------------------------------ the attack against the reference's run
@pytest.fixture(scope='module')
def golden_run():
    from arlib_amd.util.tool import seedSet
    from arlib_amd.attack.Gray.LegUP import LegUP, default_recommender_args
    g = golden('g31_legup.npz')
    seedSet(2018)
    atk = LegUP(attack_args('LegUP', 'Gray'), make_data(), rec_args=default_recommender_args(maxEpoch=1))
    atk.BiLevelOptimizationEpoch, atk.Tepoch = 2, 2
    cap = dict(tpl=[], init=None)
    orig_tpl = LegUP._template

    def template(self):
        t = orig_tpl(self)
        r, c, v = t.row.cpu().numpy(), t.col.cpu().numpy(), t.val.cpu().numpy()
        o = np.lexsort((c, r))
        cap['tpl'].append(sha(r[o].astype(np.int32), c[o].astype(np.int32), v[o].astype(np.float32)))
        return t
    from arlib_amd.attack.Gray import _gan
    orig_d = _gan.d_step

    def d_step(G, D, *a, **k):
        if cap['init'] is None:
            cap['init'] = [p.detach().cpu().numpy().copy() for p in list(G.parameters()) + list(D.parameters())]
        return orig_d(G, D, *a, **k)
    LegUP._template, _gan.d_step = template, d_step
    try:
        reseed()
        res = atk.posionDataAttack(epoch1=3, epoch2=2)
    finally:
        LegUP._template, _gan.d_step = orig_tpl, orig_d
    states = (sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8)), np.random.get_state())
    return g, atk, res, cap, states


def test_golden_exact_parts(golden_run):
    g, atk, res, cap, states = golden_run
    assert atk.targetItem == g['targets'].tolist() and atk.selectItem == g['select'].tolist()
    for n, a in zip(PARAMS, cap['init']):
        assert sha(a.astype(np.float32)) == str(g['init_sha__' + n]), n
    assert cap['tpl'] == [str(x) for x in g['tpl_sha']]
    assert [n for n, _ in atk.sample_log] == g['num_samples'].tolist()
    assert [s for _, s in atk.sample_log] == [str(x) for x in g['edge_sha']]
    assert states[0] == str(g['random_state_sha'])
    assert sha(np.asarray(states[1][1], np.uint32), np.asarray([states[1][2]], np.int64)) == str(g['numpy_state_sha'])
    for n, p in zip(PARAMS[:4], atk.G.parameters()):                                   # L_RS never reaches G: it ends where it began
        assert sha(p.detach().cpu().numpy().astype(np.float32)) == str(g['final_G_sha__' + n]) == str(g['init_sha__' + n]), n
    assert atk.lightgcn.data.user_num == atk.userNum + 8 and (atk.Tepoch, atk.batchSize, atk.attackForm) == (2, 128, 'dataAttack')
    assert atk.fakeUser == list(range(atk.userNum, atk.userNum + 9)) and res.shape == (atk.userNum + 9, atk.itemNum)


def test_golden_losses_and_discriminator(golden_run):
    """loss1 and D's final parameters: the margins test_gpu_aush.py uses for the same quantities of g30.  loss2 passes through a LightGCN training; its
    margin is that test's formula on the fixture's own spread between the reference at four torch threads and at one: max(100 * spread, 1e-5 |ref|) +
    1e-6 max |ref|.  Measured spread of g31: 0 to 8 on values of 4.45e7 to 4.51e7 (relative 1.8e-7 at most), so the bar is 450 to 850."""
    g, atk, res, cap, states = golden_run
    got = torch.cat(atk.loss_log).double().cpu().numpy()
    assert len(got) == 10
    order = [0, 1, 2, 5, 6, 7]                                                         # 3 D steps, 2 G steps, twice
    got1, got2 = got[order], got[[3, 4, 8, 9]]
    for name, gv, ref, ref1 in (('loss1', got1, g['loss1'], g['loss1_t1']), ('loss2', got2, g['loss2'], g['loss2_t1'])):
        spread = np.abs(ref - ref1)
        bar = np.maximum(100 * spread, 1e-5 * np.abs(ref)) + 1e-6 * np.abs(ref).max()
        print(name, 'got', gv.tolist(), 'ref', ref.tolist(), 'spread', spread.tolist())
        assert (np.abs(gv - ref) <= bar).all(), (name, float((np.abs(gv - ref) / bar).max()))
    for n, p in zip(PARAMS[4:], atk.D.parameters()):
        ref, ref1 = g['final_D__' + n].astype(np.float64), g['final_D_t1__' + n].astype(np.float64)
        bar = 100 * np.abs(ref - ref1).max() + 1e-4 * np.abs(ref).max()
        assert np.abs(p.detach().cpu().numpy().reshape(ref.shape) - ref).max() <= bar, n


def test_golden_fake_block(golden_run):
    g, atk, res, cap, states = golden_run
    Yg, eps = g['final_Y'], 1e-4
    assert float((np.abs(Yg - 0.1) <= eps).mean()) < 1e-3                              # the cap gen_golden_legup.py checks when it writes the fixture
    r, c, v = block(res, atk.userNum)
    got = set(zip(r.tolist(), c.tolist(), v.tolist()))
    want = set(zip(g['row'].tolist(), g['col'].tolist(), g['val'].tolist()))
    sel = np.asarray(atk.selectItem)
    near = {(int(i), int(sel[j])) for i, j in zip(*np.nonzero(np.abs(Yg - 0.1) <= eps))}
    diff = {(a, b) for a, b, _ in got ^ want}
    assert diff <= near, sorted(diff - near)


def test_second_call_reuses_generator(golden_run):
    g, atk, res, cap, states = golden_run
    n, users = len(atk.loss_log), atk.lightgcn.data.user_num
    res2 = atk.posionDataAttack()
    assert len(atk.loss_log) == n and atk.lightgcn.data.user_num == users and res2.shape == res.shape


def test_cfg2_shape_runs_without_a_score_matrix():
    """1 M users x 100 K items, d = 64, T = 5: finite loss, and peak device memory on top of the inputs stays under outputs + the kernel's workspace +
    64 MiB of slack -- less than a five-hundredth of the 400 GB a U x I fp32 matrix would take."""
    from arlib_amd import ops, _lib
    U, I, d, T = 1_000_000, 100_000, 64, 5
    g = torch.Generator(device=DEV).manual_seed(0)
    Pu, Pi = torch.randn(U, d, device=DEV, generator=g) * 0.1, torch.randn(I, d, device=DEV, generator=g) * 0.1
    cols = [20000 + t for t in range(T)]
    assert ops.colsoftmax_target_supported(U, I, d, T)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss, lse, dPu, dPi = ops.colsoftmax_target(Pu, Pi, cols, want_grad=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ws = _lib.lib().arl_colsoftmax_target_workspace_bytes(U, I, d, 1)
    bound = 4 * (U * d + I * d + I + 1) + ws + (64 << 20)
    print('cfg2 shape: loss %.6e, peak %.1f MiB, bound %.1f MiB, workspace %.1f MiB' % (float(loss), peak / 2 ** 20, bound / 2 ** 20, ws / 2 ** 20))
    assert peak <= bound and bound * 500 < 4 * U * I
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(lse).all()) and bool(torch.isfinite(dPu).all()) and bool(torch.isfinite(dPi).all())
    idx = torch.tensor([0, 20001, 99999], device=DEV)
    ref = torch.logsumexp(Pu.double() @ Pi[idx].double().t(), 0)
    assert float((lse[idx].double() - ref).abs().max()) <= 1e-5
    want = -(I * float((Pu.double().sum(0) * Pi[cols].double().sum(0)).sum()) - U * T * float(lse.double().sum()))
    assert abs(float(loss) - want) <= 1e-6 * abs(want)
    u = torch.tensor([0, 500_000, 999_999], device=DEV)
    P = torch.exp(Pu[u].double() @ Pi.double().t() - lse.double())
    ref_u = U * T * (P @ Pi.double()) - I * Pi[cols].double().sum(0)
    assert float((dPu[u].double() - ref_u).abs().max()) <= 1e-4 * float(ref_u.abs().max())

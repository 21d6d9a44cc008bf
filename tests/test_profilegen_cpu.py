"""GSPAttack's profile generator without a GPU: the C entries' exports, header comments and argument checks, the limits and predicates of
arlib_amd/profilegen.py, the composed pair-MLP route against the float64 restatement (tests/gsp_restatement.py) and against the MLP on the
concatenation, GSPAttack's two route attributes, and host tensors."""
import os
import re

import numpy as np
import pytest
import torch
from conftest import ROOT
from test_host_api import make_data
from test_shilling_cpu import attack_args
import gsp_restatement as rs

PAIR_ENTRIES = ('arl_pair_mlp_fwd_f32', 'arl_pair_mlp_bwd_f32', 'arl_pair_mlp_workspace_bytes')
GUMBEL_ENTRIES = ('arl_gumbel_topk_fwd_f32', 'arl_gumbel_topk_bwd_f32', 'arl_gumbel_topk_workspace_bytes', 'arl_gumbel_noise_f32')


def test_header_exports_and_reexports():
    from arlib_amd import _lib, ops, profilegen as pg
    hdr = open(os.path.join(ROOT, 'include', 'arlib_amd.h')).read()
    for name in PAIR_ENTRIES:
        assert name in _lib.EXPORTS and re.search(r'/\* attack/Black/GSPAttack\.py:120-130 \*/\n[^\n]*\b%s\s*\(' % name, hdr), name
    for name in GUMBEL_ENTRIES:
        assert name in _lib.EXPORTS and re.search(r'/\* attack/Black/GSPAttack\.py:201-202, 224-231 \*/\n[^\n]*\b%s\s*\(' % name, hdr), name
    assert _lib.ABI_VERSION == 34 and _lib.lib().arl_abi_version() == 34                 # the additions are additive
    for name in ('pair_mlp_logits', 'pair_mlp_logits_composed', 'pair_mlp_logits_auto', 'pair_mlp_supported', 'pair_mlp_fwd', 'pair_mlp_bwd', 'gumbel_topk',
                 'gumbel_topk_composed', 'gumbel_topk_auto', 'gumbel_topk_supported', 'gumbel_topk_fwd', 'gumbel_topk_bwd', 'gumbel_noise'):
        assert getattr(ops, name) is getattr(pg, name), name
    assert ops.PAIR_MLP_MAX_H == pg.PAIR_MLP_MAX_H >= 1024 and ops.GUMBEL_MAX_K == pg.GUMBEL_MAX_K >= 512
    # ops.py and allpairs.py only import the module: their sources define none of the new ops
    import inspect
    from arlib_amd import allpairs
    for src in (inspect.getsource(ops), inspect.getsource(allpairs)):
        assert 'def pair_mlp' not in src and 'def gumbel_' not in src


def test_supported_predicates_at_their_edges():
    from arlib_amd import profilegen as pg
    assert pg.pair_mlp_supported(60, 3706, 60) and pg.pair_mlp_supported(10_000, 100_000, 316) and pg.pair_mlp_supported(1, 1, 1)
    assert pg.pair_mlp_supported(pg.PAIR_MLP_MAX_F, pg.PROFILE_MAX_I, pg.PAIR_MLP_MAX_H)
    assert not pg.pair_mlp_supported(1, 1, pg.PAIR_MLP_MAX_H + 1) and not pg.pair_mlp_supported(1, 1, 0)
    assert not pg.pair_mlp_supported(pg.PAIR_MLP_MAX_F + 1, 1, 1) and not pg.pair_mlp_supported(0, 1, 1)
    assert not pg.pair_mlp_supported(1, pg.PROFILE_MAX_I + 1, 1) and not pg.pair_mlp_supported(1, 0, 1)
    assert pg.gumbel_topk_supported(60, 3706, 165) and pg.gumbel_topk_supported(10_000, 100_000, 32) and pg.gumbel_topk_supported(1, 1, 1)
    assert pg.gumbel_topk_supported(1, 5, 5) and not pg.gumbel_topk_supported(1, 5, 6) and not pg.gumbel_topk_supported(1, 5, 0)
    assert pg.gumbel_topk_supported(3, 1000, pg.GUMBEL_MAX_K) and not pg.gumbel_topk_supported(3, 1000, pg.GUMBEL_MAX_K + 1)
    assert not pg.gumbel_topk_supported(0, 5, 1) and not pg.gumbel_topk_supported(1, pg.PROFILE_MAX_I + 1, 1)
    assert pg.gumbel_topk_supported(2 ** 31 - 1, 256, 1) and not pg.gumbel_topk_supported(2 ** 31 - 1, 257, 1)     # F * ceil(I / 256) workgroups
    assert pg.gumbel_noise_supported(32, 64, 100_000) and not pg.gumbel_noise_supported(pg.GUMBEL_MAX_K + 1, 1, 1)
    assert not pg.gumbel_noise_supported(2, 2 ** 30, 256)


def aligned():
    buf = np.zeros(64, np.float32)
    return buf, buf.ctypes.data + (-buf.ctypes.data) % 16


def test_pair_mlp_entries_check_their_arguments_before_any_launch():
    from arlib_amd import _lib, profilegen as pg
    L = _lib.lib()
    buf, p = aligned()
    f = L.arl_pair_mlp_fwd_f32                                # (A, F, B, I, H, w2, b2, x, stream)
    for k in (0, 2, 5, 6, 7):
        a = [p, 4, p, 4, 8, p, p, p, None]
        a[k] = None
        assert f(*a) == -1, k
    assert f(p, 4, p, 4, pg.PAIR_MLP_MAX_H + 1, p, p, p, None) == -2
    assert f(p, pg.PAIR_MLP_MAX_F + 1, p, 4, 8, p, p, p, None) == -3 and f(p, 4, p, pg.PROFILE_MAX_I + 1, 8, p, p, p, None) == -3
    assert f(p, 0, p, 4, 8, p, p, p, None) == -4 and f(p, 4, p, 0, 8, p, p, p, None) == -4 and f(p, 4, p, 4, 0, p, p, p, None) == -4
    assert f(p + 4, 4, p, 4, 8, p, p, p, None) == -4 and f(p, 4, p, 4, 8, p, p, p + 4, None) == -4
    b = L.arl_pair_mlp_bwd_f32                                # (g, A, F, B, I, H, w2, dA, dB, dw2, db2, workspace, stream)
    for k in (0, 1, 3, 6, 7, 8, 9, 10, 11):
        a = [p, p, 4, p, 4, 8, p, p, p, p, p, p, None]
        a[k] = None
        assert b(*a) == -1, k
    assert b(p, p, 4, p, 4, pg.PAIR_MLP_MAX_H + 1, p, p, p, p, p, p, None) == -2
    assert b(p, p, pg.PAIR_MLP_MAX_F + 1, p, 4, 8, p, p, p, p, p, p, None) == -3
    assert b(p, p, 0, p, 4, 8, p, p, p, p, p, p, None) == -4 and b(p + 4, p, 4, p, 4, 8, p, p, p, p, p, p, None) == -4
    assert b(p, p, 4, p, 4, 8, p, p, p, p, p, p + 8, None) == -4
    w = L.arl_pair_mlp_workspace_bytes
    assert w(4, 4, pg.PAIR_MLP_MAX_H + 1) == 0 and w(0, 4, 8) == 0 and w(pg.PAIR_MLP_MAX_F + 1, 4, 8) == 0
    assert w(3, 77, 8) == 2 * 8 * 3 * 8 + 8 * 1024                               # one split of the items below 257 of them
    assert w(60, 3706, 60) == 2 * 8 * 15 * 60 * 60 + 8 * 1024                    # ml-1M: 8 row tiles x 1 column block -> 15 splits of at least 256 items
    assert w(10_000, 100_000, 316) == 2 * 8 * 10_000 * 316 + 8 * 1024            # enough workgroups without a split: O(F H)
    assert not buf.any()                                                         # nothing ran


def test_gumbel_entries_check_their_arguments_before_any_launch():
    from arlib_amd import _lib, profilegen as pg
    L = _lib.lib()
    buf, p = aligned()
    f = L.arl_gumbel_topk_fwd_f32                             # (x, F, I, k, tau, noise, seed, call, S, picks, lse, stats, workspace, stream)
    for k in (0, 8, 9, 10, 11, 12):
        a = [p, 2, 8, 3, 1.0, None, 1, 0, p, p, p, p, p, None]
        a[k] = None
        assert f(*a) == -1, k
    assert f(p, 2, 1000, pg.GUMBEL_MAX_K + 1, 1.0, None, 1, 0, p, p, p, p, p, None) == -2
    assert f(p, 2, pg.PROFILE_MAX_I + 1, 3, 1.0, None, 1, 0, p, p, p, p, p, None) == -3
    assert f(p, 2 ** 31 - 1, 257, 3, 1.0, None, 1, 0, p, p, p, p, p, None) == -3
    assert f(p, 0, 8, 3, 1.0, None, 1, 0, p, p, p, p, p, None) == -4 and f(p, 2, 8, 0, 1.0, None, 1, 0, p, p, p, p, p, None) == -4
    assert f(p, 2, 8, 9, 1.0, None, 1, 0, p, p, p, p, p, None) == -4              # k > I
    assert f(p, 2, 8, 3, 0.0, None, 1, 0, p, p, p, p, p, None) == -4 and f(p, 2, 8, 3, float('nan'), None, 1, 0, p, p, p, p, p, None) == -4
    assert f(p + 4, 2, 8, 3, 1.0, None, 1, 0, p, p, p, p, p, None) == -4 and f(p, 2, 8, 3, 1.0, p + 4, 1, 0, p, p, p, p, p, None) == -4
    b = L.arl_gumbel_topk_bwd_f32                             # (x, F, I, k, tau, noise, seed, call, picks, stats, dS, dx, workspace, stream)
    for k in (0, 8, 9, 10, 11, 12):
        a = [p, 2, 8, 3, 1.0, None, 1, 0, p, p, p, p, p, None]
        a[k] = None
        assert b(*a) == -1, k
    assert b(p, 2, 1000, pg.GUMBEL_MAX_K + 1, 1.0, None, 1, 0, p, p, p, p, p, None) == -2
    assert b(p, 2, pg.PROFILE_MAX_I + 1, 3, 1.0, None, 1, 0, p, p, p, p, p, None) == -3
    assert b(p, 2, 8, 9, 1.0, None, 1, 0, p, p, p, p, p, None) == -4 and b(p, 2, 8, 3, -1.0, None, 1, 0, p, p, p, p, p, None) == -4
    assert b(p, 2, 8, 3, 1.0, None, 1, 0, p, p, p, p + 4, p, None) == -4
    n = L.arl_gumbel_noise_f32                                # (seed, call, k, F, I, out, stream)
    assert n(1, 0, 3, 2, 8, None, None) == -1 and n(1, 0, pg.GUMBEL_MAX_K + 1, 2, 8, p, None) == -2
    assert n(1, 0, 2, 2 ** 30, 256, p, None) == -3 and n(1, 0, 3, 2, pg.PROFILE_MAX_I + 1, p, None) == -3
    assert n(1, 0, 0, 2, 8, p, None) == -4 and n(1, 0, 3, 0, 8, p, None) == -4 and n(1, 0, 3, 2, 8, p + 4, None) == -4
    w = L.arl_gumbel_topk_workspace_bytes
    assert w(2, 1000, pg.GUMBEL_MAX_K + 1, 0) == 0 and w(0, 8, 3, 0) == 0 and w(2, 8, 9, 1) == 0
    assert w(5, 1030, 41, 0) == 4 * 5 * 33 + 12                                  # a bit per item, rounded up to 16 bytes
    assert w(5, 1030, 41, 1) == (4 * 5 * 5 * 41 + 12) + (4 * 5 * 41 + 12)        # five 256-item tiles
    assert w(10_000, 100_000, 32, 0) == 4 * 10_000 * 3125                        # 125 MB beside the 4 GB of x
    assert not buf.any()


def mlp_problem(F=5, I=23, d=6, H=7, U=4, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    params = dict(mlp_w0=r(H, 2 * d), mlp_b0=r(H), mlp_w1=r(1, H), mlp_b1=r(1))
    return params, r(U + F, d), r(I, d), U


@pytest.mark.parametrize('chunk', [None, 1, 2])
def test_composed_pair_mlp_equals_the_restatement_and_the_mlp_on_the_concatenation(chunk):
    from arlib_amd import profilegen as pg
    from arlib_amd.attack.Black.GSPAttack import MLP
    params, Pu, Pi, U = mlp_problem()
    d = Pu.shape[1]
    leaves = {n: v.clone().requires_grad_() for n, v in params.items()}
    want = rs.pair_logits(leaves, Pu, Pi, U)
    up = torch.randn(want.shape, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    gw = torch.autograd.grad((want * up).sum(), list(leaves.values()))
    mine = {n: v.clone().requires_grad_() for n, v in params.items()}
    A = Pu[U:] @ mine['mlp_w0'][:, :d].t() + mine['mlp_b0']
    B = Pi @ mine['mlp_w0'][:, d:].t()
    got = pg.pair_mlp_logits_composed(A, B, mine['mlp_w1'][0], mine['mlp_b1'], chunk=chunk)
    assert got.shape == want.shape == (5, 23) and got.dtype == torch.float64
    assert float((got - want).detach().abs().max()) <= 1e-12 * float(want.detach().abs().max())
    for a, b in zip(torch.autograd.grad((got * up).sum(), list(mine.values())), gw):
        assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())
    mlp = MLP(2 * d, 7).double()
    with torch.no_grad():
        mlp.net[0].weight.copy_(params['mlp_w0']); mlp.net[0].bias.copy_(params['mlp_b0'])
        mlp.net[2].weight.copy_(params['mlp_w1']); mlp.net[2].bias.copy_(params['mlp_b1'])
        cat = torch.cat([Pu[U:, None, :].expand(5, 23, d), Pi[None].expand(5, 23, d)], 2)
        assert float((mlp(cat)[:, :, 0] - got).abs().max()) <= 1e-12 * float(want.abs().max())
    with pytest.raises(ValueError):
        pg.pair_mlp_logits_composed(A, B[:, :-1], mine['mlp_w1'][0], mine['mlp_b1'])


def test_relu_derivative_at_zero_is_zero_in_the_composed_route():
    from arlib_amd import profilegen as pg
    A = torch.tensor([[1.0, -2.0]], dtype=torch.float64, requires_grad=True)
    B = torch.tensor([[-1.0, 2.0], [0.5, 0.5]], dtype=torch.float64, requires_grad=True)       # item 0: both pre-activations exactly 0
    w2, b2 = torch.tensor([3.0, 5.0], dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    x = pg.pair_mlp_logits_composed(A, B, w2, b2)
    assert x.tolist() == [[0.0, 4.5]]
    x.sum().backward()
    assert A.grad.tolist() == [[3.0, 0.0]] and B.grad.tolist() == [[0.0, 0.0], [3.0, 0.0]]


def test_attack_route_attributes_defaults_and_rejected_values():
    from arlib_amd.attack.Black.GSPAttack import GSPAttack
    from arlib_amd.util.tool import seedSet
    seedSet(2018)
    atk = GSPAttack(attack_args('GSPAttack', 'Black', maliciousFeedbackSize=0.01, Epoch=1), make_data())
    assert atk.profile_route == 'composed' and atk.noise_source == 'torch'
    for attr, bad in (('profile_route', 'triton'), ('profile_route', None), ('noise_source', 'numpy'), ('noise_source', 'Hash')):
        good = getattr(atk, attr)
        setattr(atk, attr, bad)
        with pytest.raises(ValueError):
            atk.posionDataAttack()                                               # rejected before any device work
        setattr(atk, attr, good)
    assert atk.ngcf is None and atk.loss_log == []


def test_host_tensors_raise():
    from arlib_amd import profilegen as pg, _lib
    A, B, w2, b2 = torch.randn(3, 8), torch.randn(9, 8), torch.randn(8), torch.randn(1)
    x, noise = torch.randn(3, 9), torch.randn(2, 3, 9)
    for call in (lambda: pg.pair_mlp_logits(A, B, w2, b2), lambda: pg.pair_mlp_logits_auto(A, B, w2, b2), lambda: pg.pair_mlp_fwd(A, B, w2, b2),
                 lambda: pg.pair_mlp_bwd(x, A, B, w2, b2), lambda: pg.gumbel_topk(x, 2, noise=noise), lambda: pg.gumbel_topk(x, 2, seed=1),
                 lambda: pg.gumbel_topk_auto(x, 2, noise=noise), lambda: pg.gumbel_topk_fwd(x, 2, noise=noise),
                 lambda: pg.gumbel_noise(1, 0, 2, 3, 9, device='cpu'),
                 lambda: pg.pair_mlp_logits_auto(torch.randn(3, 1025), torch.randn(9, 1025), torch.randn(1025), b2),     # past the limits: still no CPU route
                 lambda: pg.gumbel_topk_auto(torch.randn(1, 600), 513, noise=torch.randn(513, 1, 600))):
        with pytest.raises(_lib.ArlError):
            call()

"""The multinomial likelihood on the device (csrc/arl_multinomial.hip): nll, lse, dq and dE against float64 (tests/multvae_restatement.py) at one row,
one item, ragged tiles in both directions, every width and more than one item split, with unit and with random weights, an empty and a full row; equal
bits from run to run and without gradients; exact upstream scaling; the autograd function; the dispatcher past the limits.  The poisoned-memory runs
are in test_gpu_multinomial_poison.py.

Bar for every value compared with float64 (the one test_gpu_policyhead.py and test_gpu_profilegen.py hold their kernels to): the max-norm relative
error is at most FACTOR = 4 times the composed fp32 torch route's own error on the same inputs, with FLOOR = 1e-6.  Measured figures: DESIGN.md
section 3o.

Inputs.  'plain': q ~ N(0, 1), E ~ N(0, 1 / d), so the logits are O(1).  'dominant', built as test_gpu_policyhead.py builds it: logits of standard
deviation 60 from integer-valued q and E in sixteenths (every logit is exact in fp32 in any summation order, so the comparison is about the softmax
and not about a dot product's rounding), with a near twin for every item so that the top item shares its mass; most p underflow to exactly 0 in fp32
(the online max at work)."""
import functools

import numpy as np
import pytest
import torch
import multvae_restatement as R
import stream_splits_restatement as splits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FACTOR, FLOOR = 4.0, 1e-6
SHAPES = [(1, 1, 16), (1, 33, 64), (3, 77, 16), (70, 515, 64), (130, 1030, 128), (33, 4099, 32)]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def held(what, name, got, comp, want):
    want = want.detach().numpy()
    ek, ec = rel(got.detach().cpu().numpy().reshape(want.shape), want), rel(comp.detach().cpu().numpy().reshape(want.shape), want)
    print('%s %s: kernel %.3e composed %.3e' % (what, name, ek, ec))
    assert ek <= max(FACTOR * ec, FLOOR), (what, name, ek, ec)


@functools.lru_cache(maxsize=None)
def problem(B, I, d, kind, weighted):
    g = torch.Generator().manual_seed(1000 * B + I + d + (7 if kind == 'dominant' else 0))
    q, E = torch.randn(B, d, generator=g), torch.randn(I, d, generator=g) / d ** 0.5
    if kind == 'dominant':
        q = torch.round(8 * q)
        E = torch.round(16 * (60 / (8 * d ** 0.5)) * torch.randn(I, d, generator=g)) / 16
        where = torch.randint(0, d, (I // 2, 4), generator=g)
        sign = (torch.randint(0, 2, (I // 2, 4), generator=g) * 2 - 1).float() / 16
        E[1::2] = E[0:2 * (I // 2):2] + torch.zeros(I // 2, d).scatter_add_(1, where, sign)
        assert float(q.abs().max()) <= 48 and float(E.abs().max()) < 16
    pos = torch.rand(B, I, generator=g) < 0.05
    pos[:, 0] |= ~pos.any(1)
    if B > 2:
        pos[0], pos[-1] = False, True                                  # a row without positives and a row with every item
    w = (0.25 + 2 * torch.rand(B, I, generator=g)) if weighted else None
    return q, E, pos, w, torch.randn(B, generator=g)


@functools.lru_cache(maxsize=None)
def float64(B, I, d, kind, weighted):
    return R.softmax_nll(*problem(B, I, d, kind, weighted))


def csr(pos, w=None):
    rowptr = torch.zeros(pos.shape[0] + 1, dtype=torch.int32)
    rowptr[1:] = pos.sum(1).cumsum(0)
    out = (rowptr, pos.nonzero()[:, 1].to(torch.int32)) + ((w[pos].float(),) if w is not None else ())
    return tuple(t.to(DEV) for t in out)


def on_device(B, I, d, kind='plain', weighted=False):
    q, E, pos, w, g = problem(B, I, d, kind, weighted)
    return q.to(DEV), E.to(DEV), csr(pos, w), g.to(DEV)


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'weighted'])
@pytest.mark.parametrize('kind', ['plain', 'dominant'])
@pytest.mark.parametrize('B,I,d', SHAPES)
def test_kernel_against_float64(B, I, d, kind, weighted):
    from arlib_amd import ops
    # (130, 1030) streams the items in 2 splits and (33, 4099) in 5; no shape here splits the batch rows (test_gpu_stream_splits.py does)
    assert splits.stage_splits(B, I) == splits.ITEM_SPLITS.get((B, I), (1, (I + 63) // 64 * 64)) and splits.stage_splits(I, B)[0] == 1
    q, E, P, g = on_device(B, I, d, kind, weighted)
    want = float64(B, I, d, kind, weighted)
    if kind == 'dominant' and I > 100:
        p32 = torch.softmax(q.cpu() @ E.cpu().t(), 1)
        assert float((p32 == 0).float().mean()) > 0.5                  # most p underflow to exactly 0 in fp32
    got = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    comp = ops.multinomial_softmax_composed(q, E, P, g, want_grad=True)
    again = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    fwd = ops.multinomial_softmax_kernel(q, E, P)
    what = 'multinomial B=%d I=%d d=%d %s %s' % (B, I, d, kind, 'weighted' if weighted else 'unit')
    for name, k, c, w, k2 in zip(('nll', 'lse', 'dq', 'dE'), got, comp, want, again):
        assert k.shape == c.shape and torch.equal(k, k2)               # fixed-order sums: the same bits from run to run
        assert bool(torch.isfinite(k).all())
        held(what, name, k, c, w)
    assert len(fwd) == 2 and torch.equal(fwd[0], got[0]) and torch.equal(fwd[1], got[1])     # the call without gradients runs the same arithmetic
    if B > 2:                                                          # the row without positives
        assert float(got[0][0]) == 0.0 and float(got[2][0].abs().max()) == 0.0


@pytest.mark.parametrize('B,I,d', [(3, 77, 16), (130, 1030, 128)])
def test_upstream_scales_the_gradients_exactly(B, I, d):
    from arlib_amd import ops
    q, E, P, g = on_device(B, I, d, 'plain', True)
    _, _, dq, dE = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    for s in (4.0, 0.125):
        _, _, dq2, dE2 = ops.multinomial_softmax_kernel(q, E, P, g * s, want_grad=True)
        assert torch.equal(dq2, dq * s) and torch.equal(dE2, dE * s)


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'weighted'])
@pytest.mark.parametrize('B,I,d', [(3, 77, 16), (70, 515, 64)])
def test_autograd_function_feeds_the_kernel_gradients(B, I, d, weighted):
    from arlib_amd import ops
    from arlib_amd.util.loss import multinomial_nll
    q, E, P, g = on_device(B, I, d, 'plain', weighted)
    _, _, dq64, dE64 = float64(B, I, d, 'plain', weighted)

    def run(route):
        ql, El = q.clone().requires_grad_(), E.clone().requires_grad_()
        (g * multinomial_nll(ql, El, P, route=route)).sum().backward()
        return ql.grad, El.grad
    (dq, dE), (dqc, dEc) = run('fused'), run('composed')
    held('multinomial autograd', 'dq', dq, dqc, dq64)
    held('multinomial autograd', 'dE', dE, dEc, dE64)
    direct = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    assert torch.equal(dq, direct[2]) and torch.equal(dE, direct[3])
    from arlib_amd.allpairs import transpose_positives
    again = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True, pos_t=transpose_positives(P[0], P[1], B, I))
    assert torch.equal(again[3], direct[3])                            # the caller's transposed positives are the ones built inside


@pytest.mark.parametrize('d', [24, 256])
def test_dispatcher_takes_the_composed_route_past_the_limits(d, monkeypatch):
    from arlib_amd import ops, multinomial as mn
    assert ops.multinomial_softmax is mn.multinomial_softmax
    assert not ops.multinomial_softmax_supported(9, 130, d) and ops.multinomial_softmax_supported(2048, 100_000, 64)
    taken = []
    kernel, comp = mn.multinomial_softmax_kernel, mn.multinomial_softmax_composed
    monkeypatch.setattr(mn, 'multinomial_softmax_kernel', lambda *a, **kw: (taken.append('kernel'), kernel(*a, **kw))[1])
    monkeypatch.setattr(mn, 'multinomial_softmax_composed', lambda *a, **kw: (taken.append('composed'), comp(*a, **kw))[1])
    q, E, P, g = on_device(9, 130, d, 'plain', True)
    got = mn.multinomial_softmax(q, E, P, g, want_grad=True)
    assert taken == ['composed']
    want = float64(9, 130, d, 'plain', True)
    ref = comp(q, E, P, g, want_grad=True)
    for name, k, c, w in zip(('nll', 'lse', 'dq', 'dE'), got, ref, want):
        held('multinomial dispatcher d=%d' % d, name, k, c, w)
    with pytest.raises(ValueError):
        kernel(q, E, P, g, want_grad=True)
    from arlib_amd.util.loss import multinomial_nll
    with pytest.raises(ValueError):
        multinomial_nll(q, E, P, route='fused')
    del taken[:]
    q2, E2, P2, g2 = on_device(3, 77, 16)
    mn.multinomial_softmax(q2, E2, P2, g2, want_grad=True)
    assert taken == ['kernel']


def test_arguments_are_refused_as_by_the_other_ops():
    from arlib_amd import ops
    from arlib_amd._lib import ArlError
    q, E, P, g = on_device(3, 77, 16, 'plain', True)
    with pytest.raises(ArlError):
        ops.multinomial_softmax_kernel(q.cpu(), E, P)
    with pytest.raises(ArlError):
        ops.multinomial_softmax_kernel(q, E, (P[0].cpu(), P[1], P[2]))
    with pytest.raises(ValueError):
        ops.multinomial_softmax_kernel(q, E, P, want_grad=True)         # gradients without the upstream
    with pytest.raises(ValueError):
        ops.multinomial_softmax_kernel(q, E, (P[0][:-1], P[1], P[2]))
    bad = P[1].clone()
    bad[0] = 77
    with pytest.raises(IndexError):
        ops.multinomial_softmax_kernel(q, E, (P[0], bad, P[2]))
    with pytest.raises(TypeError):
        ops.multinomial_softmax_kernel(q.double(), E.double(), P)

"""PoisonRec's policy head on the device (csrc/arl_policyhead.hip): logp, ent, dq and dE against float64 (tests/poisonrec_restatement.py) at one row,
one item, the word boundaries at 32 +- 1, ragged tiles in both directions and every width; exact upstream scaling; sampling with the caller's
uniforms and with the counter hash; the deterministic mode; run-to-run determinism; the dispatcher past the limits.  The poisoned-memory runs are
in test_gpu_policyhead_poison.py.

Bar for every value compared with float64 (the one test_gpu_profilegen.py holds its kernels to): the max-norm relative error is at most
FACTOR = 4 times the composed fp32 torch route's own error on the same inputs, with FLOOR = 1e-6.  Measured figures: DESIGN.md section 3l.

Inputs.  'plain': q ~ N(0, 1), E ~ N(0, 1 / d), so the logits are O(1).  'dominant': logits of standard deviation 60, so a row's top logit leads
the field by tens and most p underflow to exactly 0 in fp32 (sigmoid(p) = 1/2 exactly, the online max at work).  Two conditions on these inputs keep
the comparison about the head and not about a dot product's rounding: (1) q holds integers in about +-32 and E multiples of 1/16 below 16, so every
product and every partial sum of a logit fits in 19 bits and z is exact in fp32 in any summation order (a logit of size 200 rounded to fp32 in two
different orders moves p by 1e-5, the same for the kernel and for torch, and the FACTOR would then compare two draws of that noise);  (2) every
item has a near twin (E[2k + 1] = E[2k] +- 1/16 in four coordinates) whose logit is within O(1) of its own, so the top item shares the mass with
its twin and the gradients stay well conditioned (with a single surviving item every dz is an exact 0 in fp32 and a rounding residue in float64:
nothing to compare)."""
import functools

import numpy as np
import pytest
import torch
import poisonrec_restatement as rs
import stream_splits_restatement as splits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FACTOR, FLOOR = 4.0, 1e-6
SHAPES = [(1, 1, 16), (1, 33, 64), (3, 77, 16), (70, 515, 64), (130, 1030, 128), (33, 4099, 32)]
GAP = 1e-5


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def held(what, name, got, comp, want):
    want = want.detach().numpy()
    ek, ec = rel(got.detach().cpu().numpy().reshape(want.shape), want), rel(comp.detach().cpu().numpy().reshape(want.shape), want)
    print('%s %s: kernel %.3e composed %.3e' % (what, name, ek, ec))
    assert ek <= max(FACTOR * ec, FLOOR), (what, name, ek, ec)


@functools.lru_cache(maxsize=None)
def problem(B, I, d, kind, acts='random'):
    g = torch.Generator().manual_seed(1000 * B + I + d + (7 if kind == 'dominant' else 0))
    q, E = torch.randn(B, d, generator=g), torch.randn(I, d, generator=g) / d ** 0.5
    if kind == 'dominant':
        q = torch.round(8 * q)
        E = torch.round(16 * (60 / (8 * d ** 0.5)) * torch.randn(I, d, generator=g)) / 16
        where = torch.randint(0, d, (I // 2, 4), generator=g)
        sign = (torch.randint(0, 2, (I // 2, 4), generator=g) * 2 - 1).float() / 16
        E[1::2] = E[0:2 * (I // 2):2] + torch.zeros(I // 2, d).scatter_add_(1, where, sign)
        assert float(q.abs().max()) <= 48 and float(E.abs().max()) < 16
    a = torch.rand(B, I, generator=g) < 0.5
    if acts == 'zeros':
        a[:] = False
    elif acts == 'ones':
        a[:] = True
    elif B > 2:
        a[0], a[-1] = False, True                                  # an all-zero and an all-one row among the random ones
    gl, ge = torch.randn(B, generator=g), torch.randn(B, generator=g)
    u = torch.rand(B, I, generator=g)
    return q, E, a, gl, ge, u


@functools.lru_cache(maxsize=None)
def float64(B, I, d, kind, acts='random'):
    q, E, a, gl, ge, _ = problem(B, I, d, kind, acts)
    return rs.head(q, E, a, gl, ge)


def on_device(B, I, d, kind, acts='random'):
    from arlib_amd import ops
    q, E, a, gl, ge, u = problem(B, I, d, kind, acts)
    words = rs.pack(a.numpy()).to(DEV)
    assert torch.equal(ops.pack_bits(a.to(DEV)), words)
    return q.to(DEV), E.to(DEV), words, gl.to(DEV), ge.to(DEV), u.to(DEV)


CASES = [(B, I, d, kind, 'random') for (B, I, d) in SHAPES for kind in ('plain', 'dominant')] + \
        [(B, I, d, 'plain', acts) for (B, I, d) in ((1, 33, 64), (3, 77, 16)) for acts in ('zeros', 'ones')]


@pytest.mark.parametrize('B,I,d,kind,acts', CASES)
def test_eval_against_float64(B, I, d, kind, acts):
    from arlib_amd import ops
    # (130, 1030) streams the items in 2 splits and (33, 4099) in 5, in the statistics passes and in dq alike; no shape here splits the batch rows
    # (test_gpu_stream_splits.py does)
    assert splits.ph_item_splits(I) == splits.stage_splits(B, I) == splits.ITEM_SPLITS.get((B, I), (1, (I + 63) // 64 * 64))
    assert splits.stage_splits(I, B)[0] == 1
    q, E, words, gl, ge, _ = on_device(B, I, d, kind, acts)
    logp64, ent64, dq64, dE64, p64 = float64(B, I, d, kind, acts)
    if kind == 'dominant' and I > 100:
        p32 = torch.softmax(q @ E.t(), 1)
        assert float((p32 == 0).float().mean()) > 0.5                 # most p underflow to exactly 0 in fp32
    got = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    comp = ops.bernoulli_softmax_eval_composed(q, E, words, gl, ge, want_grad=True)
    again = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    fwd = ops.bernoulli_softmax_eval(q, E, words)
    what = 'head B=%d I=%d d=%d %s %s' % (B, I, d, kind, acts)
    for name, k, c, w, k2 in zip(('logp', 'ent', 'dq', 'dE'), got, comp, (logp64, ent64, dq64, dE64), again):
        assert k.shape == c.shape and torch.equal(k, k2)              # fixed-order sums: the same bits from run to run
        held(what, name, k, c, w)
    assert torch.equal(fwd[0], got[0]) and torch.equal(fwd[1], got[1])  # the call without gradients runs the same arithmetic


@pytest.mark.parametrize('B,I,d', [(3, 77, 16), (70, 515, 64)])
def test_autograd_function_feeds_the_kernel_gradients(B, I, d):
    from arlib_amd import ops
    q, E, words, gl, ge, _ = on_device(B, I, d, 'plain')
    _, _, dq64, dE64, _ = float64(B, I, d, 'plain')

    def run(route):
        ql, El = q.clone().requires_grad_(), E.clone().requires_grad_()
        logp, ent = ops.bernoulli_softmax_head(ql, El, words, route=route)
        (gl * logp + ge * ent).sum().backward()
        return ql.grad, El.grad
    (dq, dE), (dqc, dEc) = run('fused'), run('composed')
    held('head autograd', 'dq', dq, dqc, dq64)
    held('head autograd', 'dE', dE, dEc, dE64)
    direct = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    assert torch.equal(dq, direct[2]) and torch.equal(dE, direct[3])


@pytest.mark.parametrize('B,I,d', [(3, 77, 16), (130, 1030, 128)])
def test_upstreams_scale_the_gradients_exactly(B, I, d):
    from arlib_amd import ops
    q, E, words, gl, ge, _ = on_device(B, I, d, 'plain')
    _, _, dq, dE = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    for s in (4.0, 0.125):
        _, _, dq2, dE2 = ops.bernoulli_softmax_eval(q, E, words, gl * s, ge * s, want_grad=True)
        assert torch.equal(dq2, dq * s) and torch.equal(dE2, dE * s)
    zero = torch.zeros_like(ge)
    a = ops.bernoulli_softmax_eval(q, E, words, gl, zero, want_grad=True)
    b = ops.bernoulli_softmax_eval(q, E, words, gl, -zero, want_grad=True)
    logp64, ent64, dq64, dE64, _ = rs.head(q.cpu(), E.cpu(), problem(B, I, d, 'plain')[2], gl.cpu(), zero.cpu())
    comp = ops.bernoulli_softmax_eval_composed(q, E, words, gl, zero, want_grad=True)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    held('head gl only', 'dq', a[2], comp[2], dq64)
    held('head gl only', 'dE', a[3], comp[3], dE64)


def redrawn(u, sg64, gen):
    """Redraw every u whose float64 gap |u - sigmoid(p)| is below GAP: a condition on the inputs, which leaves no case out."""
    u = u.clone()
    while True:
        near = (u.double() - sg64).abs() < GAP
        if not bool(near.any()):
            return u
        u[near] = torch.rand(int(near.sum()), generator=gen)


@pytest.mark.parametrize('B,I,d,kind', [(B, I, d, kind) for (B, I, d) in SHAPES for kind in ('plain', 'dominant')])
def test_sampling_with_the_callers_uniforms(B, I, d, kind):
    from arlib_amd import ops
    q, E, _, _, _, u = problem(B, I, d, kind)
    sg64 = rs.sample(q, E, u)[4]
    u = redrawn(u, sg64, torch.Generator().manual_seed(B + I))
    a64, logp64, count64, gap, _ = rs.sample(q, E, u)
    print('sample B=%d I=%d d=%d %s: smallest float64 gap %.3e' % (B, I, d, kind, gap))
    assert gap >= GAP
    qd, Ed, ud = q.to(DEV), E.to(DEV), u.to(DEV)
    words, logp, count = ops.bernoulli_softmax_sample(qd, Ed, u=ud)
    wc, logpc, countc = ops.bernoulli_softmax_sample_composed(qd, Ed, u=ud)
    assert words.dtype == torch.int32 and words.shape == (B, (I + 31) // 32)
    assert torch.equal(words.cpu(), rs.pack(a64.numpy()))             # bit for bit, pad bits 0
    assert torch.equal(wc, words) and torch.equal(count.cpu().long(), count64) and torch.equal(countc, count)
    held('sample B=%d I=%d d=%d %s' % (B, I, d, kind), 'logp', logp, logpc, logp64)
    again = ops.bernoulli_softmax_sample(qd, Ed, u=ud)
    assert all(torch.equal(x, y) for x, y in zip((words, logp, count), again))
    # the evaluation of the sampled actions gives the sampler's log-probability (the same arithmetic)
    assert torch.equal(ops.bernoulli_softmax_eval(qd, Ed, words)[0], logp)


@pytest.mark.parametrize('B,I,d', [(3, 77, 16), (33, 4099, 32), (70, 515, 64)])
def test_sampling_with_the_counter_hash(B, I, d):
    from arlib_amd import ops
    q, E, _, _, _, _ = problem(B, I, d, 'plain')
    qd, Ed = q.to(DEV), E.to(DEV)
    seed, call = 2 ** 63 + 12345, 7
    u = ops.bernoulli_uniforms(seed, call, B, I, device=DEV)
    assert u.shape == (B, I) and float(u.min()) >= 0.0 and float(u.max()) < 1.0 and 0.4 < float(u.mean()) < 0.6
    assert not torch.equal(u, ops.bernoulli_uniforms(seed, call + 1, B, I, device=DEV))
    for b in (0, B - 1):                                              # a function of (seed, call, row0 + b, i) only
        assert torch.equal(ops.bernoulli_uniforms(seed, call, 1, I, row0=b, device=DEV)[0], u[b])
    words, logp, count = ops.bernoulli_softmax_sample(qd, Ed, seed=seed, call=call)
    for b in range(B):                                                # a B-row call = B single-row calls with row0 = b, bit for bit
        w1, l1, c1 = ops.bernoulli_softmax_sample(qd[b:b + 1], Ed, seed=seed, call=call, row0=b)
        assert torch.equal(w1[0], words[b]) and torch.equal(l1[0], logp[b]) and torch.equal(c1[0], count[b])
    a64, _, count64, gap, sg64 = rs.sample(q, E, u.cpu())
    near = (u.cpu().double() - sg64).abs() < GAP                      # the same gap condition: positions this close are left out of the comparison
    got = ops.unpack_bits(words, I).cpu()
    assert int(near.sum()) <= 1 + B * I // 1000 and torch.equal(got[~near], a64[~near])
    wu = ops.bernoulli_softmax_sample(qd, Ed, u=u)
    assert all(torch.equal(x, y) for x, y in zip((words, logp, count), wu))       # the kernel's hash draw is the written-out draw


def levels_problem(B, I, d):
    """Logits on fixed levels: q_b = 64 e_(b % d) and E[i, k] = level((i + k) % 6) / 64, so z[b, i] is a level exactly.  p = exp(level) / sum: the levels
    0, -1, -5, -60 keep p above 1e-30 (a normal fp32 number), -130 and -800 put it below 1e-50 (0 in fp32): no p lies between, where fp32 and float64
    could disagree about p > 0."""
    lv = torch.tensor([0.0, -1.0, -5.0, -60.0, -130.0, -800.0])
    q = torch.zeros(B, d)
    q[torch.arange(B), torch.arange(B) % d] = 64.0
    E = lv[(torch.arange(I)[:, None] + torch.arange(d)[None]) % 6] / 64.0
    return q, E


@pytest.mark.parametrize('B,I,d', [(1, 33, 64), (3, 77, 16), (70, 515, 64)])
def test_deterministic_mode_picks_the_items_with_positive_p(B, I, d):
    from arlib_amd import ops
    q, E = levels_problem(B, I, d)
    p64 = torch.softmax(q.double() @ E.double().t(), 1)
    assert not bool(((p64 > 1e-50) & (p64 < 1e-30)).any()) and bool((p64 < 1e-50).any()) and bool((p64 > 1e-30).any())
    words, logp, count = ops.bernoulli_softmax_sample(q.to(DEV), E.to(DEV), deterministic=True)
    want = p64 > 1e-30
    assert torch.equal(words.cpu(), rs.pack(want.numpy())) and torch.equal(count.cpu().long(), want.sum(1))
    wc, logpc, countc = ops.bernoulli_softmax_sample_composed(q.to(DEV), E.to(DEV), deterministic=True)
    assert torch.equal(wc, words) and torch.equal(countc, count)
    logp64 = rs.head(q, E, want)[0]
    held('deterministic B=%d I=%d' % (B, I), 'logp', logp, logpc, logp64)
    # plain inputs: every p is positive, so every item is picked
    q2, E2, _, _, _, _ = problem(B, I, d, 'plain')
    w2, _, c2 = ops.bernoulli_softmax_sample(q2.to(DEV), E2.to(DEV), deterministic=True)
    assert c2.tolist() == [I] * B and torch.equal(w2.cpu(), rs.pack(np.ones((B, I), bool)))


def test_dispatcher_and_limits():
    from arlib_amd import ops, policyhead
    assert not ops.bernoulli_softmax_supported(4, 50, 48) and ops.bernoulli_softmax_supported(10_000, 100_000, 64)
    g = torch.Generator().manual_seed(5)
    q, E = torch.randn(4, 48, generator=g).to(DEV), (torch.randn(50, 48, generator=g) / 7).to(DEV)
    a = torch.rand(4, 50, generator=g) < 0.5
    words, gl, ge = ops.pack_bits(a.to(DEV)), torch.ones(4, device=DEV), torch.ones(4, device=DEV)
    logp, ent, dq, dE = ops.bernoulli_softmax(q, E, words, gl, ge, want_grad=True)           # d = 48: the composed route
    want = rs.head(q.cpu(), E.cpu(), a, gl.cpu(), ge.cpu())
    for got, w in zip((logp, ent, dq, dE), want):
        assert rel(got.cpu().numpy(), w.numpy()) < 1e-5
    sw, sl, sc = ops.bernoulli_softmax_sample_auto(q, E, deterministic=True)
    assert sc.tolist() == [50] * 4
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_eval(q, E, words)
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_sample(q, E, deterministic=True)
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_head(q, E, words, route='fused')
    q16, E16 = q[:, :16].contiguous(), E[:, :16].contiguous()
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_eval(q16, E16, words[:, :1])                                   # the wrong number of action words
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_sample(q16, E16)                                               # neither u nor seed
    with pytest.raises(ValueError):
        ops.bernoulli_softmax_eval(q16, E16, words, want_grad=True)                          # gradients without upstreams
    assert policyhead.bernoulli_softmax is ops.bernoulli_softmax

"""The attacks' hot path at its edges: the CW term (arl_cw_topk_term_f32: cw_user / cw_scan / cw_fill / cw_item / cw_finish) on multi-slice item
groups, odd widths, degenerate lists and magnitudes, its limits and the row-primitive fallback past them (attack._common.cw_term), and the
second form of score_mask_topk's stream at its wave / workgroup / stage / bootstrap edges, incl. warm starts for users with fewer than k unmasked
items.  Every result is held against float64 (torch double on the device) and, where the path is deterministic, against a second run bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
from conftest import close

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ARL_E_DIM, ARL_E_RANGE, ARL_E_ARG = -2, -3, -4


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on the MI355X box)')
    from arlib_amd import ops as _ops
    return _ops


def ipg(d):
    return 128 if d <= 128 else 64


# ------------------------------------------------------------------------------------------------ CW term

def cw_ref64(X, Up, n_real, top, targets, c=None):
    """float64 CW term (attack/White/CLeaR.py:84-95 as a sum over (real user, target) pairs, negative = the list's k-1-t-th entry): loss, G, w, and
    the sum of the loss's terms' magnitudes (the scale its fp32 rounding error lives on: the terms have both signs)."""
    Xd = X.double()
    N, d = Xd.shape
    I, k, T = N - Up, top.shape[1], targets.numel()
    c = 1.0 / (max(n_real, 1) * T) if c is None else c
    tg = targets.long()
    G = torch.zeros_like(Xd)
    w = torch.zeros(N, dtype=torch.float64, device=X.device)
    loss = torch.zeros((), dtype=torch.float64, device=X.device)
    mag = 0.0
    if n_real:
        ue = Xd[:n_real]
        neg = top[:n_real, k - T:].flip(1).long()
        sum_u = ue.sum(0)
        for t in range(T):
            xn = Xd[Up + neg[:, t]]
            loss += c * ((ue * xn).sum() - (sum_u * Xd[Up + tg[t]]).sum())
            mag += c * ((ue * xn).sum(1).abs().sum() + (ue @ Xd[Up + tg[t]]).abs().sum()).item()
            G[:n_real] += c * (xn - Xd[Up + tg[t]])
            G[Up:].index_add_(0, neg[:, t], c * ue)
            G[Up + tg[t]] -= c * sum_u
        w[:n_real] = T
        w[Up:] += torch.bincount(neg.reshape(-1), minlength=I).double()
        w[Up:].index_add_(0, tg, torch.full((T,), float(n_real), dtype=torch.float64, device=X.device))
    return loss, G, w, mag


def check_cw(got, ref, Up, n_real, loss_tol=1e-5):
    """loss within loss_tol of the float64 term's magnitude, G by close() on the user rows and on the item rows separately (their magnitudes differ
    by up to 60 orders in the scaled cases), w exactly."""
    loss, G, w = got
    rl, rG, rw, mag = ref
    scale = max(abs(rl.item()), mag, 1e-300)
    assert abs(loss.double().item() - rl.item()) <= loss_tol * scale or (rl.item() == 0.0 and loss.item() == 0.0), (loss.item(), rl.item())
    for a, b in ((G[:Up], rG[:Up]), (G[Up:], rG[Up:])):
        if bool((b != 0).any()):
            assert close(a.cpu().numpy(), b.cpu().numpy())
        else:
            assert not bool(a.any())
    if w is not None:
        assert torch.equal(w, rw.float())


def max_group_entries(top, n_real, T, d):
    k = top.shape[1]
    neg = top[:n_real, k - T:].long().reshape(-1)
    return int(torch.bincount(neg // ipg(d)).max()) if neg.numel() else 0


def run_twice(ops, X, Up, n_real, top, tg, **kw):
    a = ops.cw_topk_term(X, Up, n_real, top, tg, **kw)
    b = ops.cw_topk_term(X, Up, n_real, top, tg, **kw)
    assert all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))            # deterministic: bit for bit
    return a


def tables(seed, Up, I, d, scale=0.1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    X = torch.randn(Up + I, d, device=DEV, generator=g) * scale
    return X, g


@pytest.mark.parametrize('case', ['one_group', 'one_item', 'spread'])
def test_cw_term_multi_slice_groups(ops, case):
    """Item groups with more than kCwSlice = 8 192 entries: cw_scan_kernel's slice table has several slices for one group and cw_item_kernel merges
    their fixed-point partials with 64-bit global atomics.  The test asserts that the largest group does exceed one slice."""
    d, F = 64, 17
    if case == 'one_group':                  # 40 000 users, T = 5, 90 % of the negatives on the 128 items of one group
        n_real, I, k, T = 40_000, 20_000, 20, 5
    elif case == 'one_item':                 # one item closes every list: > 8 192 entries on a single row
        n_real, I, k, T = 20_000, 5_000, 10, 3
    else:                                    # spread: every group holds several slices
        n_real, I, k, T = 60_000, 3_000, 16, 8
    Up = n_real + F
    X, g = tables({'one_group': 1, 'one_item': 2, 'spread': 3}[case], Up, I, d)
    top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
    if case == 'one_group':
        g0 = 37
        hot = (torch.rand(n_real, T, device=DEV, generator=g) < 0.9)
        inside = torch.randint(g0 * 128, g0 * 128 + 128, (n_real, T), device=DEV, generator=g, dtype=torch.int32)
        top[:n_real, k - T:] = torch.where(hot, inside, top[:n_real, k - T:])
    elif case == 'one_item':
        top[:, k - 1] = 1234
    tg = torch.tensor([0, I - 1, 500][:T] + list(range(7, 7 + max(0, T - 3))), dtype=torch.int64, device=DEV)
    assert max_group_entries(top, n_real, T, d) > 8192
    got = run_twice(ops, X, Up, n_real, top, tg)
    check_cw(got, cw_ref64(X, Up, n_real, top, tg), Up, n_real)


@pytest.mark.parametrize('d', [4, 12, 252, 256])
def test_cw_term_widths(ops, d):
    """Widths off the usual 64 / 128: d = 4 and 12 (cw_user_kernel's 4- and 8-lane rows), 252 and 256 (64-lane rows, groups of 64 items, four
    64-column passes of cw_item_kernel, 128 KB of LDS accumulators), with a group over one slice."""
    n_real, F, I, k, T = 12_000, 9, 1_000, 12, 4
    Up = n_real + F
    X, g = tables(d, Up, I, d)
    top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
    top[:, k - 1] = I - 1
    tg = torch.tensor([0, I - 1, 3, 999 % I], dtype=torch.int64, device=DEV)
    assert max_group_entries(top, n_real, T, d) > 8192
    check_cw(run_twice(ops, X, Up, n_real, top, tg), cw_ref64(X, Up, n_real, top, tg), Up, n_real)


@pytest.mark.parametrize('k', [7, 64])
def test_cw_term_every_list_entry_a_negative(ops, k):
    """T = k: every entry of every list is popped (the deepest pop reads rank 0), including a target repeated in the target list."""
    n_real, F, I, d = 3_000, 5, 900, 64
    Up = n_real + F
    X, g = tables(k, Up, I, d)
    top = torch.stack([torch.randperm(I, device=DEV, generator=g)[:k] for _ in range(Up)]).to(torch.int32)
    tl = list(range(0, 2 * k, 2)); tl[1] = tl[0]
    tg = torch.tensor(tl, dtype=torch.int64, device=DEV)
    check_cw(run_twice(ops, X, Up, n_real, top, tg), cw_ref64(X, Up, n_real, top, tg), Up, n_real)


def test_cw_term_no_real_users(ops):
    """n_real = 0 with fake rows: no pairs -- the loss is 0 and G and w are 0 on every row (the formula with empty sums), on the kernel and on
    the fallback."""
    from arlib_amd.attack._common import cw_term_rows
    F, I, d, k = 40, 300, 64, 10
    X, g = tables(3, F, I, d)
    top = torch.randint(0, I, (F, k), device=DEV, generator=g, dtype=torch.int32)
    tg = torch.tensor([1, 2, 2], dtype=torch.int64, device=DEV)
    for loss, G, w in (run_twice(ops, X, F, 0, top, tg), cw_term_rows(X, F, 0, top, tg)):
        assert loss.item() == 0.0 and not bool(G.any()) and not bool(w.any())


@pytest.mark.parametrize('d', [64, 256])
@pytest.mark.parametrize('off', [-1, 0, 1])
def test_cw_term_item_count_at_group_boundary(ops, d, off):
    """I = ipg * m + off: the last group full, exactly full, or holding one item; the last item is a target and a popular negative."""
    I = ipg(d) * 5 + off
    n_real, F, k, T = 10_000, 3, 8, 3
    Up = n_real + F
    X, g = tables(I + d, Up, I, d)
    top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
    top[: n_real // 2, k - 1] = I - 1
    tg = torch.tensor([I - 1, 0, I // 2], dtype=torch.int64, device=DEV)
    check_cw(run_twice(ops, X, Up, n_real, top, tg), cw_ref64(X, Up, n_real, top, tg), Up, n_real)


@pytest.mark.parametrize('mode', ['tiny', 'huge', 'zero', 'spanning'])
def test_cw_term_user_row_magnitudes(ops, mode):
    """The fixed-point exponent of cw_scan_kernel follows the real users' largest magnitude: rows scaled by 1e-30 and 1e30 push it to either end,
    all-zero rows leave it at 0, rows spanning 1e-6 ... 1e2 put small addends next to large ones in one item sum."""
    n_real, F, I, d, k, T = 20_000, 6, 700, 64, 10, 5
    Up = n_real + F
    X, g = tables(7, Up, I, d)
    if mode == 'tiny':
        X[:n_real] *= 1e-30
    elif mode == 'huge':
        X[:n_real] *= 1e30
    elif mode == 'zero':
        X[:n_real] = 0.0
    else:
        X[:n_real] *= 10.0 ** (torch.rand(n_real, 1, device=DEV, generator=g) * 8 - 6)
    top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
    top[:, k - 1] = 5
    tg = torch.tensor([0, 1, 2, 3, I - 1], dtype=torch.int64, device=DEV)
    assert max_group_entries(top, n_real, T, d) > 8192
    loss, G, w = run_twice(ops, X, Up, n_real, top, tg)
    assert bool(torch.isfinite(G).all())
    ref = cw_ref64(X, Up, n_real, top, tg)
    check_cw((loss, G, w), ref, Up, n_real)
    if mode == 'zero':
        assert loss.item() == 0.0 and not bool(G[Up:].any())


# ------------------------------------------------------------------------------------------------ limits and the fallback

def raw_cw(ops, X, Up, n_real, top, tg):
    """arl_cw_topk_term_f32 called directly (no shape checks of the wrapper): (return code, loss, G, w)."""
    from arlib_amd import _lib
    L = _lib.lib()
    N, d = X.shape
    I, T = N - Up, tg.numel()
    ws = torch.empty(max(L.arl_cw_topk_term_workspace_bytes(I, d, n_real, T), 8), dtype=torch.uint8, device=DEV)
    G, loss, w = torch.empty_like(X), torch.empty(1, device=DEV), torch.empty(N, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = L.arl_cw_topk_term_f32(p(X), Up, I, d, n_real, p(top), top.shape[1], p(tg), T, 1.0 / (max(n_real, 1) * T), p(G), p(loss), p(w), p(ws), ops._stream())
    torch.cuda.synchronize()
    return rc, loss, G, w


@pytest.mark.parametrize('d,I_max', [(64, 1_048_576), (256, 524_288)])
def test_cw_term_item_limit_kernel_then_fallback(ops, d, I_max):
    """8 192 item groups: the kernel takes I_max items (the C entry returns ARL_OK and the float64 term), rejects I_max + 1 before any launch
    (ARL_E_RANGE; cw_topk_term_supported agrees on both sides), and attack._common.cw_term gives the same term there through the fallback."""
    from arlib_amd.attack._common import cw_term
    from arlib_amd._lib import ArlError
    n_real, F, k, T = 3_000, 40, 12, 5
    Up = n_real + F
    for I, want in ((I_max, True), (I_max + 1, False)):
        X, g = tables(I, Up, I, d)
        top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
        top[:n_real // 3, k - 1] = I - 1                                          # the last group, with more than one slice
        tg = torch.tensor([0, I - 1, I // 2, 77, I - 2], dtype=torch.int64, device=DEV)
        assert ops.cw_topk_term_supported(I, d, T, k) is want
        rc, loss, G, w = raw_cw(ops, X, Up, n_real, top, tg)
        ref = cw_ref64(X, Up, n_real, top, tg)
        if want:
            assert rc == 0
            check_cw((loss, G, w), ref, Up, n_real)
        else:
            assert rc == ARL_E_RANGE
            with pytest.raises(ArlError):
                ops.cw_topk_term(X, Up, n_real, top, tg)
        check_cw(cw_term(X, Up, n_real, top, tg), ref, Up, n_real)
        del X, G, ref
        torch.cuda.empty_cache()


@pytest.mark.parametrize('T,k', [(64, 64), (65, 80), (100, 100)])
def test_cw_term_target_limit_kernel_then_fallback(ops, T, k):
    """T <= 64 targets on the kernel; T = 65 and 100 with k >= T rejected by the C entry before any launch (ARL_E_ARG), and the same term through
    the fallback -- deterministic, with a repeated target; T > k raises on both routes."""
    from arlib_amd.attack._common import cw_term
    n_real, F, I, d = 2_000, 7, 1_500, 64
    Up = n_real + F
    X, g = tables(T + k, Up, I, d)
    top = torch.stack([torch.randperm(I, device=DEV, generator=g)[:k] for _ in range(Up)]).to(torch.int32)
    tl = list(range(3, 3 + 7 * T, 7)); tl[5] = tl[2]
    tg = torch.tensor(tl, dtype=torch.int64, device=DEV)
    ref = cw_ref64(X, Up, n_real, top, tg)
    supported = T <= 64
    assert ops.cw_topk_term_supported(I, d, T, k) is supported
    rc = raw_cw(ops, X, Up, n_real, top, tg)[0]
    assert rc == (0 if supported else ARL_E_ARG)
    a, b = cw_term(X, Up, n_real, top, tg), cw_term(X, Up, n_real, top, tg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    check_cw(a, ref, Up, n_real)
    with pytest.raises(ValueError):
        cw_term(X, Up, n_real, top[:, :T - 1].contiguous(), tg)
    with pytest.raises(ValueError):
        ops.cw_topk_term(X, Up, n_real, top[:, :T - 1].contiguous(), tg)
    assert raw_cw(ops, X, Up, n_real, top[:, :T - 1].contiguous(), tg)[0] == ARL_E_ARG


@pytest.mark.parametrize('d', [256, 258, 260])
def test_cw_term_width_limit(ops, d):
    """d <= 256 and d % 4 == 0: the predicate and the C entry agree (the other widths are rejected before any launch and go to the fallback)."""
    from arlib_amd.attack._common import cw_term
    n_real, F, I, k, T = 500, 3, 200, 8, 3
    Up = n_real + F
    X, g = tables(d, Up, I, d)
    top = torch.randint(0, I, (Up, k), device=DEV, generator=g, dtype=torch.int32)
    tg = torch.tensor([0, 1, I - 1], dtype=torch.int64, device=DEV)
    supported = ops.cw_topk_term_supported(I, d, T, k)
    assert supported is (d == 256)
    rc = raw_cw(ops, X, Up, n_real, top, tg)[0]
    assert rc == (0 if supported else ARL_E_DIM)
    check_cw(cw_term(X, Up, n_real, top, tg), cw_ref64(X, Up, n_real, top, tg), Up, n_real)


def _attack_problem(T, k):
    """Tables, an interaction mask and the masked top-k lists of the scalar top-k kernel (k > 64)."""
    from arlib_amd import ops
    g = torch.Generator(device=DEV).manual_seed(70)
    n_real, F, I, d = 300, 4, 500, 16
    Up = n_real + F
    Pu = torch.randn(Up, d, device=DEV, generator=g, dtype=torch.float64) * 0.3
    Pi = torch.randn(I, d, device=DEV, generator=g, dtype=torch.float64) * 0.3
    lens = torch.randint(0, 30, (Up,), generator=torch.Generator().manual_seed(1))
    cols = [np.sort(np.random.default_rng(u).choice(I, int(lens[u]), replace=False)).astype(np.int32) for u in range(Up)]
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum(lens.numpy())]).astype(np.int32)).to(DEV)
    mc = torch.from_numpy(np.concatenate(cols)).to(DEV)
    top, _ = ops.score_mask_topk(Pu.float().contiguous(), Pi.float().contiguous(), k, rp, mc)
    targets = list(range(1, 1 + 7 * T, 7))
    return Pu, Pi, top, n_real, targets


def _reference_cw(Pu, Pi, top, n_real, targets):
    """CLeaR.py:84-95 / BiLevelAttackByBatchInject.py:80-92 literally, in float64: pairs (user, target, popped negative), mean of neg - pos scores."""
    T, k = len(targets), top.shape[1]
    users = torch.arange(n_real, device=DEV).repeat_interleave(T)
    pos = torch.tensor(targets, device=DEV).repeat(n_real)
    neg = top[users, k - 1 - torch.arange(T, device=DEV).repeat(n_real)].long()
    ue, pe, ne = Pu[users], Pi[pos], Pi[neg]
    return ((ue * ne).sum(1) - (ue * pe).sum(1)).mean(), (ue, pe, ne)


def test_bilevel_cw_loss_past_the_target_limit():
    """BiLevelAttackByBatchInject's CW loss at T = 70 targets, k = 80 (the kernel group stops at 64 targets): loss and table gradients against
    float64 autograd of the reference expression."""
    from arlib_amd.attack.White.BiLevelAttackByBatchInject import _CwLoss
    Pu, Pi, top, n_real, targets = _attack_problem(70, 80)
    pu, pi = Pu.float().requires_grad_(True), Pi.float().requires_grad_(True)
    loss = _CwLoss.apply(pu, pi, top, n_real, targets)
    gu, gi = torch.autograd.grad(loss, (pu, pi))
    Pu.requires_grad_(True); Pi.requires_grad_(True)
    ref, _ = _reference_cw(Pu, Pi, top, n_real, targets)
    ru, ri = torch.autograd.grad(ref, (Pu, Pi))
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item())
    assert close(gu.cpu().numpy(), ru.cpu().numpy()) and close(gi.cpu().numpy(), ri.cpu().numpy())


def test_clear_cw_sfa_loss_past_the_target_limit():
    """CLeaR's CW + SFA losses at T = 70, k = 80: the CW term, the SFA term (its row multiplicities come from the fallback's w) and the table
    gradients of their sum against float64 autograd of CLeaR.py:84-126 with the same r0."""
    from arlib_amd.attack.White.CLeaR import _CwSfaLoss
    Pu, Pi, top, n_real, targets = _attack_problem(70, 80)
    r0 = torch.randn(Pu.shape[1], generator=torch.Generator().manual_seed(5), dtype=torch.float64).to(DEV)
    pu, pi = Pu.float().requires_grad_(True), Pi.float().requires_grad_(True)
    cw, sfa = _CwSfaLoss.apply(pu, pi, top, n_real, torch.tensor(targets, device=DEV), r0.float())
    gu, gi = torch.autograd.grad(cw + sfa, (pu, pi))
    Pu.requires_grad_(True); Pi.requires_grad_(True)
    rcw, (ue, pe, ne) = _reference_cw(Pu, Pi, top, n_real, targets)
    H = torch.cat([ue, pe, ne], 0)
    r = H.T @ (H @ r0)
    rsfa = torch.nn.functional.l1_loss(H - (H @ torch.outer(r, r)) / torch.norm(r) ** 2, H)
    ru, ri = torch.autograd.grad(rcw + rsfa, (Pu, Pi))
    assert abs(cw.item() - rcw.item()) <= 1e-5 * abs(rcw.item())
    assert abs(sfa.item() - rsfa.item()) <= 1e-4 * abs(rsfa.item())
    assert close(gu.cpu().numpy(), ru.cpu().numpy()) and close(gi.cpu().numpy(), ri.cpu().numpy())


# ------------------------------------------------------------------------------------------------ score_mask_topk, second form

def topk_ref64(Pu, Pi, k, cols):
    """Stable float64 argsort of the masked scores (interacted = -10e8, as the reference): ids and values of the top k, lowest id first on ties."""
    sc = Pu.double() @ Pi.double().T
    for u, c in enumerate(cols):
        if len(c):
            sc[u, torch.from_numpy(c).to(DEV).long()] = -10e8
    v, i = torch.sort(sc, dim=1, descending=True, stable=True)
    return i[:, :k].to(torch.int32), v[:, :k]


def check_near_ties(idx, val, ridx, rval):
    """The existing allowance: ids identical except where two scores tie within the split contraction's rounding; values within 2e-6 of the
    largest unmasked score, masked entries (-10e8) exactly where float64 has them."""
    free = rval > -5e8
    assert torch.equal(val > -5e8, free)
    if bool(free.any()):
        scale = max(1e-3, rval[free].abs().max().item())
        assert (val.double() - rval)[free].abs().max().item() <= 2e-6 * scale
    assert bool((val[~free] == -10e8).all())
    same = idx == ridx
    for r, c in torch.nonzero(~same).tolist():
        assert abs(rval[r, c].item() - val[r, c].item()) <= 1e-5 * max(1.0, abs(rval[r, c].item()))
    assert same.float().mean().item() > 0.995


def both_forms(ops, Pu, Pi, k, rp, mc, warm=None):
    out = []
    for form2 in (False, True):
        ops.TOPK_FORM2 = form2
        ops.reset_exit_probe()
        try:
            out.append(ops.score_mask_topk(Pu, Pi, k, rp, mc, warm_idx=warm))
        finally:
            ops.TOPK_FORM2 = True
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    return out[1]


def mask_of(cols):
    if not sum(len(c) for c in cols):
        return None, None
    rp = torch.from_numpy(np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)).to(DEV)
    flat = np.concatenate(cols) if sum(len(c) for c in cols) else np.zeros(1, np.int32)
    return rp, torch.from_numpy(flat.astype(np.int32)).to(DEV)


@pytest.mark.parametrize('k,U,I', [(2, 1, 2), (10, 31, 127), (20, 33, 129), (32, 513, 32_767), (33, 513, 32_768), (63, 33, 32_769),
                                   (10, 513, 32_769), (20, 1, 32_768), (63, 513, 63), (33, 31, 129), (2, 33, 32_767), (32, 1, 127)])
def test_score_mask_topk_second_form_edges(ops, k, U, I):
    """d = 64, both forms of the fp16 stream bit for bit (cold and warm) and against float64, at k around a wave's 32 users and the 64-lane
    lists, U around 32-user waves and 512-user workgroups, I = k, around a 128-item stage and the bootstrap switch at 32 768 -- with the rows that
    go wrong first: a zero user row (the k lowest-id unmasked items, all exactly 0), users with exactly k, k - 1 and 0 unmasked items, and a heavy
    user with ~20 000 masked items (its Bloom filter saturates: every candidate takes the binary search)."""
    rng = np.random.default_rng(1000 * k + U + I)
    d = 64
    Pu = torch.from_numpy((rng.standard_normal((U, d)) * 0.1).astype(np.float32)).to(DEV)
    Pi = torch.from_numpy((rng.standard_normal((I, d)) * 0.1 * (rng.pareto(2.0, I) + 0.1)[:, None]).astype(np.float32)).to(DEV)
    cols = [np.sort(rng.choice(I, int(rng.integers(0, min(40, I // 2) + 1)), replace=False)).astype(np.int32) for _ in range(U)]
    special = {}
    if U >= 5:
        special = {0: 'zero', 1: 'k', 2: 'k-1', 3: 'none', 4: 'heavy' if I >= 20_000 + k else 'k'}
    elif U == 1:
        special = {0: 'zero'}
    for u, kind in special.items():
        if kind == 'zero':
            Pu[u] = 0.0
            cols[u] = np.sort(rng.choice(I, min(I - k, 3), replace=False)).astype(np.int32)
        elif kind in ('k', 'k-1'):
            cols[u] = np.sort(rng.choice(I, I - k + (kind == 'k-1'), replace=False)).astype(np.int32)
        elif kind == 'none':
            cols[u] = np.arange(I, dtype=np.int32)
        else:
            cols[u] = np.sort(rng.choice(I, 20_000, replace=False)).astype(np.int32)
    rp, mc = mask_of(cols)
    ridx, rval = topk_ref64(Pu, Pi, k, cols)
    idx, val = both_forms(ops, Pu, Pi, k, rp, mc)
    check_near_ties(idx, val, ridx, rval)
    for u, kind in special.items():
        if kind == 'zero':
            free = np.setdiff1d(np.arange(I), cols[u])[:k]
            assert np.array_equal(idx[u].cpu().numpy(), free) and bool((val[u] == 0).all())
        else:
            assert torch.equal(idx[u], ridx[u]) or kind == 'heavy'
    i_w, v_w = both_forms(ops, Pu, Pi, k, rp, mc, warm=idx)
    assert torch.equal(i_w, idx) and torch.equal(v_w, val)
    i_n, v_n = both_forms(ops, Pu, Pi, k, None, None)
    check_near_ties(i_n, v_n, *topk_ref64(Pu, Pi, k, [np.zeros(0, np.int32)] * U))


@pytest.mark.parametrize('d,form2', [(64, True), (64, False), (32, False), (128, False)])
def test_score_mask_topk_warm_start_with_short_users_needs_no_cold_repeat(ops, d, form2):
    """Users with fewer than k unmasked items (k - 1, a handful, none): their lists end in masked items (-10e8), which no threshold from the warm
    candidates' unmasked scores lets through -- such a user starts at -inf.  A warm call from the cold result equals it bit for bit WITHOUT raising
    the underflow flag (no cold repeat); invalid candidates on a full user still raise it, and the repeat still gives the cold result."""
    rng = np.random.default_rng(d + form2)
    U, I, k = 600, 3000, 50
    Pu = torch.from_numpy((rng.standard_normal((U, d)) * 0.1).astype(np.float32)).to(DEV)
    Pi = torch.from_numpy((rng.standard_normal((I, d)) * 0.1).astype(np.float32)).to(DEV)
    lens = rng.integers(0, 60, U)
    lens[::7] = I - k + 1
    lens[3::7] = I - 5
    lens[5::7] = I
    lens[6::7] = I - k                                                        # exactly k unmasked: a full list, the flag stays armed
    cols = [np.sort(rng.choice(I, int(n), replace=False)).astype(np.int32) for n in lens]
    rp, mc = mask_of(cols)
    saved = dict(ops.TOPK_STATS)
    ops.TOPK_FORM2 = form2
    ops.TOPK_STATS['record_events'] = True
    try:
        ops.TOPK_STATS['flags'] = []
        cold_i, cold_v = ops.score_mask_topk(Pu, Pi, k, rp, mc)
        w_i, w_v = ops.score_mask_topk(Pu, Pi, k, rp, mc, warm_idx=cold_i)
        bad = cold_i.clone(); bad[:, 1:] = bad[:, :1]
        b_i, b_v = ops.score_mask_topk(Pu, Pi, k, rp, mc, warm_idx=bad)
        flags = [int(f.item()) for f in ops.TOPK_STATS['flags']]
    finally:
        ops.TOPK_FORM2 = True
        ops.TOPK_STATS.clear(); ops.TOPK_STATS.update(saved)
    assert torch.equal(w_i, cold_i) and torch.equal(w_v, cold_v)
    assert torch.equal(b_i, cold_i) and torch.equal(b_v, cold_v)
    assert flags == [0, 1], flags
    ridx, rval = topk_ref64(Pu, Pi, k, cols)
    check_near_ties(cold_i, cold_v, ridx, rval)
    short = np.nonzero(I - lens < k)[0]
    assert len(short) > 100 and bool((cold_v[torch.from_numpy(short).to(DEV), -1] <= -5e8).all())

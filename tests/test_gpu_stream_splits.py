"""The streamed kernels where their host split rules change (csrc/arl_stream.h): the shapes here exist for their split structure, and every case
first asserts that structure through tests/stream_splits_restatement.py (which test_stream_splits_cpu.py pins to the built library), so a retuned
rule fails the case instead of emptying it.

Multinomial likelihood and policy head with the BATCH ROWS streamed in splits (B > 1 024: mn_stream_kernel<D, MN_DE> and ph_stream_kernel<D, PH_DE>
with blockIdx.y > 0, the part_dE sections, the folds over them), one shape with both directions split in one call.  Bar, unchanged: the max-norm
relative error against float64 is at most FACTOR = 4 times the composed fp32 route's on the same inputs, FLOOR = 1e-6 (held() of the families' own
files).  The upstream of the seam rows (the last row of every split, the first of the next, row B - 1) is 16 times the drawn one and their
coefficients are non-zero in float64, so a seam row that is dropped or counted twice shows in dE; each case prints the smallest share one seam
row alone has of dE (max |dz_b| max |q_b| / max |dE| in float64; 5e-5 to 1 over the cases, measured against bars of 1e-6 to 2.5e-5 and at least
three times the bar of its own case).  Measured figures: DESIGN.md section 3q.

Target rank with targets and ties on the seams of the item splits: a target on the first and last item of a stage, of a split, alone in the last
split, masked items on both sides of a seam, on normal tables (the bracket of rank_restatement), integer tables (exact) and a table where every
score ties (exact: the number of unmasked items below the target, the one input where the kernel's switch from >= to > decides every count)."""
import functools

import numpy as np
import pytest
import torch
import multvae_restatement as MR
import poisonrec_restatement as PR
import rank_restatement as RK
import stream_splits_restatement as S
import test_gpu_multinomial as MN
import test_gpu_policyhead as PH
from test_targetrank_cpu import tens

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SEAM_GAIN = 16.0                                                       # a power of two: the scaled upstream is exact
ROW_SHAPES = sorted(S.ROW_SPLIT_SHAPES)


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')


def assert_row_splits(B, I, d, item_rule):
    """The split structure the shape exists for; returns the seam rows of the streamed batch rows."""
    sb, last = S.ROW_SPLIT_SHAPES[(B, I, d)]
    assert S.stage_splits(I, B) == sb and sb[0] > 1 and S.last_len(B, sb) == last
    if (B, I, d) == S.BOTH_SPLIT_SHAPE:
        sq, last_items = S.BOTH_ITEM_SPLIT
        assert S.stage_splits(B, I) == item_rule(B, I) == sq and sq[0] > 1 and S.last_len(I, sq) == last_items
    else:
        assert S.stage_splits(B, I)[0] == item_rule(B, I)[0] == 1
    return S.seam_rows(B, sb)


def seam_shares(dz, q, dE, seams):
    """max |dz_b| max |q_b| / max |dE| of each seam row b, in float64: the largest entry of the row's own term dz_b^T q_b against the whole sum."""
    return [float(dz[b].abs().max() * q[b].abs().max() / dE.abs().max()) for b in seams]


# ------------------------------------------------------------------------------------------------ multinomial likelihood
@functools.lru_cache(maxsize=None)
def mn_case(B, I, d, kind, weighted):
    """(q, E, pos, w, g with the seam rows' upstream scaled, float64 outputs, the seam rows' shares of dE); computed once, never modified."""
    q, E, pos, w, g = MN.problem(B, I, d, kind, weighted)
    seams = S.seam_rows(B, S.stage_splits(I, B))
    g = g.clone()
    g[seams] *= SEAM_GAIN
    want = MR.softmax_nll(q, E, pos, w, g)
    A = pos.double() if w is None else w.double() * pos.double()
    coef = g.double() * A.sum(1)                                       # the row's dense coefficient g_b n_b
    dz = coef[:, None] * torch.softmax(q.double() @ E.double().t(), 1) - g.double()[:, None] * A
    return q, E, pos, w, g, want, coef[seams], seam_shares(dz, q.double(), want[3], seams)


@pytest.mark.parametrize('weighted', [False, True], ids=['unit', 'weighted'])
@pytest.mark.parametrize('kind', ['plain', 'dominant'])
@pytest.mark.parametrize('B,I,d', ROW_SHAPES)
def test_multinomial_with_the_batch_rows_in_splits(B, I, d, kind, weighted):
    from arlib_amd import ops, _lib
    seams = assert_row_splits(B, I, d, lambda B, I: S.stage_splits(B, I))
    assert int(_lib.lib().arl_multinomial_softmax_workspace_bytes(B, I, d, 1)) == S.multinomial_softmax_workspace_bytes(B, I, d, True)
    q, E, pos, w, g, want, coef, shares = mn_case(B, I, d, kind, weighted)
    what = 'multinomial B=%d I=%d d=%d %s %s' % (B, I, d, kind, 'weighted' if weighted else 'unit')
    print('%s: seam rows %s, smallest share of dE %.3e' % (what, seams, min(shares)))
    assert bool((coef != 0).all()) and min(shares) > 0
    q, E, P, g = q.to(DEV), E.to(DEV), MN.csr(pos, w), g.to(DEV)
    got = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    comp = ops.multinomial_softmax_composed(q, E, P, g, want_grad=True)
    again = ops.multinomial_softmax_kernel(q, E, P, g, want_grad=True)
    fwd = ops.multinomial_softmax_kernel(q, E, P)
    for name, k, c, w64, k2 in zip(('nll', 'lse', 'dq', 'dE'), got, comp, want, again):
        assert k.shape == c.shape and torch.equal(k, k2)               # fixed-order sums: the same bits from run to run
        assert bool(torch.isfinite(k).all())
        MN.held(what, name, k, c, w64)
    assert len(fwd) == 2 and torch.equal(fwd[0], got[0]) and torch.equal(fwd[1], got[1])     # the call without gradients runs the same arithmetic
    assert float(got[0][0]) == 0.0 and float(got[2][0].abs().max()) == 0.0                   # the row without positives


# ------------------------------------------------------------------------------------------------ policy head
@functools.lru_cache(maxsize=None)
def ph_case(B, I, d, kind):
    """(q, E, actions, gl and ge with the seam rows' upstreams scaled, float64 outputs, the seam rows' largest |dz| and shares of dE)."""
    q, E, a, gl, ge, _ = PH.problem(B, I, d, kind)
    seams = S.seam_rows(B, S.stage_splits(I, B))
    gl, ge = gl.clone(), ge.clone()
    gl[seams] *= SEAM_GAIN
    ge[seams] *= SEAM_GAIN
    logp, ent, dq, dE, p = PR.head(q, E, a, gl, ge)
    sg = 1 / (1 + torch.exp(-p))
    c = gl.double()[:, None] * (a.double() - sg) - ge.double()[:, None] * p * sg * (1 - sg)
    dz = p * (c - (p * c).sum(1, keepdim=True))                        # the module's own formula for dz; dE = dz^T q
    assert PH.rel(dz.t() @ q.double(), dE) < 1e-12
    return q, E, a, gl, ge, (logp, ent, dq, dE), dz[seams].abs().amax(1), seam_shares(dz, q.double(), dE, seams)


@pytest.mark.parametrize('kind', ['plain', 'dominant'])
@pytest.mark.parametrize('B,I,d', ROW_SHAPES)
def test_policy_head_with_the_batch_rows_in_splits(B, I, d, kind):
    from arlib_amd import ops, _lib
    seams = assert_row_splits(B, I, d, lambda B, I: S.ph_item_splits(I))
    assert int(_lib.lib().arl_bernoulli_softmax_workspace_bytes(B, I, d, 1)) == S.bernoulli_softmax_workspace_bytes(B, I, d, True)
    q, E, a, gl, ge, want, coef, shares = ph_case(B, I, d, kind)
    what = 'head B=%d I=%d d=%d %s' % (B, I, d, kind)
    print('%s: seam rows %s, smallest share of dE %.3e' % (what, seams, min(shares)))
    assert bool((gl[seams] != 0).all()) and bool((ge[seams] != 0).all()) and bool((coef > 0).all()) and min(shares) > 0
    words = PR.pack(a.numpy()).to(DEV)
    q, E, gl, ge = q.to(DEV), E.to(DEV), gl.to(DEV), ge.to(DEV)
    got = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    comp = ops.bernoulli_softmax_eval_composed(q, E, words, gl, ge, want_grad=True)
    again = ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    fwd = ops.bernoulli_softmax_eval(q, E, words)
    for name, k, c, w64, k2 in zip(('logp', 'ent', 'dq', 'dE'), got, comp, want, again):
        assert k.shape == c.shape and torch.equal(k, k2)               # fixed-order sums: the same bits from run to run
        PH.held(what, name, k, c, w64)
    assert torch.equal(fwd[0], got[0]) and torch.equal(fwd[1], got[1])  # the call without gradients runs the same arithmetic


# ------------------------------------------------------------------------------------------------ target rank
# (U, I, T, d, seed, targets in this order, the two items either side of a seam that one user's mask gains)
RANK_CASES = [(3, 4097, 8, 64, 31, [4096, 0, 63, 64, 511, 512, 4095, 2048], (511, 512)),
              (17, 1025, 6, 16, 32, [383, 384, 767, 768, 1024, 0], (383, 384))]
RANK_IDS = ['U%d_I%d' % c[:2] for c in RANK_CASES]
MASK_USER = 2


def with_items(mask, u, items):
    """The CSR mask with `items` added to user u's list (sorted, distinct)."""
    rowptr, col = mask
    rows = [sorted(set(col[rowptr[r]:rowptr[r + 1]].tolist()) | (set(items) if r == u else set())) for r in range(len(rowptr) - 1)]
    out = np.zeros(len(rowptr), np.int32)
    out[1:] = np.cumsum([len(r) for r in rows])
    return out, np.array([c for r in rows for c in r], np.int32)


@functools.lru_cache(maxsize=None)
def rank_case(k, masked, table):
    U, I, T, d, seed, targets, extra = RANK_CASES[k]
    Pu, Pi, _ = RK.draw_case(U, I, T, d, seed, integer=table != 'normal')
    if table == 'ties':
        Pu = np.zeros_like(Pu)
    targets = np.array(targets, np.int32)
    mask = with_items(RK.draw_mask(U, I, targets, seed), MASK_USER, extra) if masked else None
    return Pu, Pi, targets, mask, RK.restate(Pu, Pi, targets, mask)


@pytest.mark.parametrize('table', ['normal', 'integer', 'ties'])
@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masked'])
@pytest.mark.parametrize('k', range(len(RANK_CASES)), ids=RANK_IDS)
def test_target_rank_with_targets_and_ties_on_the_seams(k, masked, table):
    from arlib_amd import ops, _lib
    U, I, T, d, _, tg, extra = RANK_CASES[k]
    (ns, length), last = S.RANK_SPLIT_SHAPES[(U, I)]
    assert S.trk_splits(U, I) == (ns, length) and ns > 1 and S.last_len(I, (ns, length)) == last and len(tg) == T
    assert int(_lib.lib().arl_target_rank_workspace_bytes(U, I, d, T)) == S.up16(4 * ns * U * T)
    # the places the targets are there for: both ends of the table, of the first seam and of the last seam (at I = 4097 the last split's only item)
    assert {0, length - 1, length, (ns - 1) * length - 1, (ns - 1) * length, I - 1} <= set(tg) and extra == (length - 1, length)
    assert any(t % 64 == 63 for t in tg) and any(t % 64 == 0 for t in tg)
    Pu, Pi, targets, mask, ref = rank_case(k, masked, table)
    if masked:
        lst = mask[1][mask[0][MASK_USER]:mask[0][MASK_USER + 1]].tolist()
        assert extra[0] in lst and extra[1] in lst
    if table == 'ties':
        # every score is 0: the rank is the number of unmasked items with a smaller id, written out without the restatement
        M = RK.dense_mask(mask[0], mask[1], U, I) if masked else np.zeros((U, I), bool)
        below = np.concatenate([np.zeros((U, 1), np.int64), np.cumsum(~M, 1)], 1)[:, targets]
        assert np.array_equal(ref['rank0'], np.where(M[:, targets], -1, below))
    rank, ts = ops.target_rank_kernel(tens(Pu, DEV), tens(Pi, DEV), tens(targets, DEV), (tens(mask[0], DEV), tens(mask[1], DEV)) if masked else None)
    rank, ts = rank.cpu().numpy(), ts.cpu().numpy()
    if table == 'normal':
        assert RK.check_bracket(rank, ref) == []
        assert (np.abs(ts.astype(np.float64) - ref['tscore']) <= ref['tbound']).all()
    else:
        assert np.array_equal(rank, ref['rank0']), '%d pairs differ' % int((rank != ref['rank0']).sum())
        assert np.array_equal(ts.astype(np.float64), ref['tscore'])

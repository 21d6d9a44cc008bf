"""Float64 restatement of the target-rank op (arlib_amd/targetrank.py, csrc/arl_targetrank.hip) and of the metrics that follow from it.  A helper,
not collected.

For fp32 tables, S = Pu Pi^T in float64 and A = |Pu| |Pi|^T, any fp32 evaluation of a score is within gamma * A of S, gamma = (d + 2) * 2^-24 (the
dot-product rounding bound for any summation order).  Two scores are compared, so a candidate may disagree with float64 about `s[u, j] > s[u, t]`
only where |S[u, j] - S[u, t]| <= tau[u, j, t] = gamma (A[u, j] + A[u, targets[t]]).  Hence for every valid pair
    lo[u, t] = #{ S[u, j] > S[u, t] + tau }  <=  rank[u, t]  <=  hi[u, t] = #{ S[u, j] >= S[u, t] - tau },      j != targets[t], (u, j) unmasked,
and at tau = 0 with ties broken by item id the count is the rank itself (`rank0`): on integer tables every fp32 route is exact and must give it."""
import numpy as np

# (U, I, T, d, seed): across the 16-row wave, the 64-row block and stage, the target groups of 8 / 16 / 32 / 64, and a split item stream
CASES = [(1, 1, 1, 16, 11), (17, 129, 5, 32, 12), (130, 1000, 17, 16, 13), (130, 1000, 17, 128, 20), (65, 4097, 64, 64, 20), (200, 1000, 8, 32, 16)]
IDS = ['U%d_I%d_T%d_d%d' % c[:4] for c in CASES]


def gamma(d):
    return (d + 2) * 2.0 ** -24


def draw_case(U, I, T, d, seed, integer=False):
    """(Pu [U, d], Pi [I, d], targets [T]): standard normal tables, or integer ones from {-2, ..., 2} (every fp32 route exact, ties everywhere)."""
    rng = np.random.default_rng(seed)
    if integer:
        Pu, Pi = rng.integers(-2, 3, (U, d)).astype(np.float32), rng.integers(-2, 3, (I, d)).astype(np.float32)
    else:
        Pu, Pi = rng.standard_normal((U, d)).astype(np.float32), rng.standard_normal((I, d)).astype(np.float32)
    targets = np.sort(rng.choice(I, T, replace=False)).astype(np.int32) if seed % 2 else rng.choice(I, T, replace=False).astype(np.int32)
    return Pu, Pi, targets


def draw_mask(U, I, targets, seed):
    """CSR (rowptr [U + 1], col [nnz]) int32, rows sorted and distinct: each user lists 0 to 40 random items; every third user also lists one or two
    targets; user 0 lists all targets; user 1 (when there is one) lists nothing."""
    rng = np.random.default_rng(seed + 1000)
    rows = []
    for u in range(U):
        n = min(int(rng.integers(0, 41)), I)
        s = set(rng.choice(I, n, replace=False).tolist())
        if u % 3 == 2:
            s |= set(rng.choice(targets, min(len(targets), 1 + u % 2), replace=False).tolist())
        if u == 0:
            s |= set(targets.tolist())
        if u == 1:
            s = set()
        rows.append(sorted(s))
    rowptr = np.zeros(U + 1, np.int32)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.array([c for r in rows for c in r], np.int32)
    return rowptr, col


def dense_mask(rowptr, col, U, I):
    M = np.zeros((U, I), bool)
    rows = np.repeat(np.arange(U), np.diff(rowptr))
    M[rows, col] = True
    return M


def restate(Pu, Pi, targets, mask=None):
    """dict of lo, hi, rank0 (int64 [U, T]; rank0 = -1 where the target is listed), listed (bool [U, T]), tscore and tbound (float64 [U, T]: S and
    gamma * A at the targets)."""
    U, d = Pu.shape
    I, T = Pi.shape[0], len(targets)
    P, Q = Pu.astype(np.float64), Pi.astype(np.float64)
    S, A = P @ Q.T, np.abs(P) @ np.abs(Q).T
    g = gamma(d)
    M = dense_mask(mask[0], mask[1], U, I) if mask is not None else np.zeros((U, I), bool)
    ids = np.arange(I)
    lo, hi, rank0 = (np.zeros((U, T), np.int64) for _ in range(3))
    for t, tg in enumerate(targets.tolist()):
        st = S[:, tg:tg + 1]
        tau = g * (A + A[:, tg:tg + 1])
        count = ~M & (ids != tg)[None, :]
        lo[:, t] = (count & (S > st + tau)).sum(1)
        hi[:, t] = (count & (S >= st - tau)).sum(1)
        rank0[:, t] = (count & ((S > st) | ((S == st) & (ids < tg)[None, :]))).sum(1)
    listed = M[:, targets]
    rank0[listed] = -1
    return {'lo': lo, 'hi': hi, 'rank0': rank0, 'listed': listed, 'tscore': S[:, targets], 'tbound': g * A[:, targets]}


def metrics_from_ranks(R, ks, valid=None):
    """The numbers of util.metrics.TargetRankMetric in float64 from a rank matrix R [U, T] (pairs outside `valid` skipped; default R >= 0)."""
    R = np.asarray(R, np.int64)
    U, T = R.shape
    v = (R >= 0) if valid is None else valid
    out = {'hitRate': [], 'precision': [], 'recall': [], 'NDCG': [], 'exposure': []}
    for k in ks:
        b = v & (R < k)
        disc = 1.0 / np.log2(2.0 + np.arange(k))
        out['hitRate'].append(float((b.any(1) / T).sum() / U))
        out['precision'].append(float(b.sum() / (U * k)))
        out['recall'].append(float(b.sum() / (U * T)))
        out['NDCG'].append(float(disc[R[b]].sum() / (disc[:min(k, T)].sum() * U)))
        with np.errstate(invalid='ignore', divide='ignore'):
            out['exposure'].append(float(np.nanmean(b.sum(0) / v.sum(0))) if v.any() else float('nan'))
    out['meanRank'] = float((R[v] + 1.0).mean()) if v.any() else float('nan')
    out['MRR'] = float((1.0 / (R[v] + 1.0)).mean()) if v.any() else float('nan')
    return out


def check_bracket(rank, ref):
    """Violations of lo <= rank <= hi on the valid pairs and of the -1 positions (empty list = fine)."""
    rank = np.asarray(rank, np.int64)
    bad = []
    if not np.array_equal(rank == -1, ref['listed']):
        bad.append('-1 positions differ at %d pairs' % int(((rank == -1) != ref['listed']).sum()))
    v = ~ref['listed']
    out = v & ((rank < ref['lo']) | (rank > ref['hi']))
    if out.any():
        u, t = np.argwhere(out)[0]
        bad.append('%d pairs outside [lo, hi], first (u %d, t %d): rank %d, lo %d, hi %d' % (int(out.sum()), u, t, rank[u, t], ref['lo'][u, t], ref['hi'][u, t]))
    return bad

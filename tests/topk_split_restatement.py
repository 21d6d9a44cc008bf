"""numpy restatement of the fp16-split contraction of score_mask_topk (arl_kernels.hip: split_scale, split_f16x2_kernel, the three-product
score) and the checks of its contract, shared by tests/test_topk_split_cpu.py and tests/test_gpu_topk_range.py.

The restatement: one power-of-two scale per table (clamped to 2^+-40), every scaled element cut into a high and a low float16 piece, the three
products ah*bh + ah*bl + al*bh (each exact in fp32) summed in float64, scaled back.  It leaves out the kernel's fp32 summation, so its error is
the split's alone."""
import numpy as np

SPREAD_LOG2 = 16          # kSplitSpreadLog2: the split is used while every nonzero row's largest |element| is within 2^-16 of its table's
EXP_LO, EXP_HI = -27, 53  # exponents of a table's largest magnitude for which split_scale is not clamped


def gamma(d):
    """Per-pair bound of the contract: |val - float64 score| <= gamma(d) |a| |b| (any-order fp32 dot product + the dropped al*bl term)."""
    return d * 2.0 ** -24 + 2.0 ** -21


def split_scale(m):
    """split_scale of the kernel for a table whose largest magnitude is the float32 m."""
    e = int(np.float32(m).view(np.uint32)) >> 23 & 0xff
    if e == 0 or e >= 255:
        return 1.0
    return 2.0 ** (min(max(127 + 13 - (e - 127), 127 - 40), 127 + 40) - 127)


def split_pieces(X):
    """(high, low, scale): the two float16 pieces of the scaled table, as float64, and the table's scale."""
    X = np.asarray(X, np.float32)
    s = split_scale(np.abs(X).max() if X.size else 0.0)
    with np.errstate(over='ignore', under='ignore'):
        x = X * np.float32(s)
        h = x.astype(np.float16)
        l = (x - h.astype(np.float32)).astype(np.float16)
    return h.astype(np.float64), l.astype(np.float64), s


def split_scores(Pu, Pi):
    """The three-product scores of every pair, float64 [U, I]."""
    ah, al, su = split_pieces(Pu)
    bh, bl, si = split_pieces(Pi)
    return (ah @ bh.T + ah @ bl.T + al @ bh.T) * ((1.0 / su) * (1.0 / si))


def table_in_contract(X):
    """split_table_ok of the kernel: the table's exponent inside the clamp and every nonzero row's largest |element| within 2^-SPREAD_LOG2 of the table's."""
    X = np.asarray(X, np.float32)
    rm = np.abs(X).max(axis=1)
    m = rm.max() if rm.size else np.float32(0)
    if m == 0:
        return True
    e = (int(np.float32(m).view(np.uint32)) >> 23 & 0xff) - 127
    if not EXP_LO <= e <= EXP_HI:
        return False
    return bool(rm[rm > 0].min().astype(np.float64) * 2.0 ** SPREAD_LOG2 >= float(m))


def pair_error(scores, Pu, Pi):
    """max over pairs of |scores - float64 scores| / (|a| |b|) (pairs with a zero row: the absolute error, which must then be 0)."""
    a, b = np.asarray(Pu, np.float64), np.asarray(Pi, np.float64)
    nn = np.linalg.norm(a, axis=1)[:, None] * np.linalg.norm(b, axis=1)[None, :]
    err = np.abs(scores - a @ b.T)
    return float((err / np.where(nn > 0, nn, 1.0)).max())


def reference_topk(Pu, Pi, k, cols=None):
    """float64 scores (masked entries at -10e8, as the kernels write them) and the stable descending top-k ids."""
    sc = np.asarray(Pu, np.float64) @ np.asarray(Pi, np.float64).T
    if cols is not None:
        for u, c in enumerate(cols):
            sc[u, c] = -10e8
    return sc, stable_topk(sc, k)


def stable_topk(sc, k):
    """np.argsort(-sc, axis=1, kind='stable')[:, :k] without sorting whole rows: ties in table order, lowest id first."""
    I = sc.shape[1]
    kth = np.partition(sc, I - k, axis=1)[:, I - k]
    ridx = np.empty((sc.shape[0], k), np.int64)
    for u in range(sc.shape[0]):
        cand = np.nonzero(sc[u] >= kth[u])[0]
        ridx[u] = cand[np.argsort(-sc[u, cand], kind='stable')[:k]]
    return ridx


def list_figures(idx, val, ref, ridx, Pu, Pi, g):
    """One result against the float64 lists, as figures: 'worst' = max over returned pairs of |val - ref| / (g |a| |b|) (entries the reference holds
    at -10e8 aside: 'masked_ok' says they ARE -10e8), 'lost' = items of the float64 list that are missing from ours WITHOUT being near-ties of what
    took their place (ref[u,i] - ref[u,j] > g |a| (|b_i| + |b_j|) for some item j of ours that float64 does not list; masked entries waived on either
    side), 'share' = share of list positions that differ from float64's, 'descending', 'distinct', 'nan'."""
    nu, ni = np.linalg.norm(np.asarray(Pu, np.float64), axis=1), np.linalg.norm(np.asarray(Pi, np.float64), axis=1)
    idx = np.clip(idx.astype(np.int64), 0, len(ni) - 1)
    r = np.take_along_axis(ref, idx, 1)
    masked = r <= -5e8
    bound = g * nu[:, None] * ni[idx]
    err = np.abs(val.astype(np.float64) - r)
    rel = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))      # (a zero row: the score must be exactly 0)
    srt = np.sort(idx, axis=1)
    diff = idx != ridx
    lost = 0
    for u in np.nonzero(diff.any(axis=1))[0]:
        ours, theirs = set(idx[u].tolist()), set(ridx[u].tolist())
        gone = [i for i in theirs - ours if ref[u, i] > -5e8]
        extra = [j for j in ours - theirs if ref[u, j] > -5e8]
        if gone and extra:
            floor = min(ref[u, j] + g * nu[u] * ni[j] for j in extra)
            lost += sum(ref[u, i] - g * nu[u] * ni[i] > floor for i in gone)
    return {'worst': float(rel[~masked].max()) if (~masked).any() else 0.0, 'masked_ok': bool((val[masked] == np.float32(-10e8)).all()), 'lost': int(lost),
            'share': float(diff.mean()), 'descending': bool((val[:, :-1] >= val[:, 1:]).all()), 'distinct': bool((srt[:, 1:] != srt[:, :-1]).all()),
            'nan': bool(np.isnan(val).any())}


def check_lists(idx, val, ref, ridx, Pu, Pi, g, cap=0.005):
    """The contract on one result (list_figures): no NaN, distinct ids in range, descending values, the value bound for every returned pair, the
    near-tie rule for every item float64 lists and we do not, and at most `cap` of the positions differing from float64's at all."""
    assert (idx >= 0).all() and (idx < Pi.shape[0]).all()
    f = list_figures(idx, val, ref, ridx, Pu, Pi, g)
    assert not f['nan'] and f['distinct'] and f['descending'] and f['masked_ok'], f
    assert f['worst'] <= 1.0, 'value bound: worst pair at %.3g of it' % f['worst']
    assert f['lost'] == 0, '%d items lost that are no near-ties' % f['lost']
    assert f['share'] <= cap, 'near-ties excused: %.4f of the positions' % f['share']
    return f

"""The contract of arlib_amd.userknn.uknn_score_topk restated in pure Python: a dict accumulator of Python ints per user, filled slot by slot
from the neighbour's set, a sort on (-score, id) tuples, the target ranks read off the sorted list.  Slow on purpose and free of numpy
arithmetic, so that it shares nothing with the kernel or the host route.  The inputs come from tests/cooccur_restatement.py."""
import numpy as np
import scipy.sparse as sp

from cooccur_restatement import sets_of, planted, identical_rows  # noqa: F401  (re-exported for the tests)


def uknn_score_topk(interact, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None):
    S = sets_of(interact)
    n_items = sp.csr_matrix(interact).shape[1]
    ni, nw = np.asarray(nbr_idx).tolist(), np.asarray(nbr_w).tolist()
    queries = list(range(len(S))) if rows is None else [int(r) for r in rows]
    tg = None if targets is None else [int(t) for t in targets]
    idx, score = np.full((len(queries), N), -1, np.int32), np.zeros((len(queries), N), np.int64)
    rank = None if tg is None else np.full((len(queries), len(tg)), -1, np.int32)
    for q, u in enumerate(queries):
        acc = {}
        for v, w in zip(ni[u], nw[u]):                      # as written: a neighbour in two slots counts twice, u itself counts
            if v >= 0:
                for i in S[v]:
                    acc[i] = acc.get(i, 0) + int(w)
        cand = sorted((-acc.get(i, 0), i) for i in range(n_items) if not (mask_profile and i in S[u]))
        for j, (s, i) in enumerate(cand[:N]):
            idx[q, j], score[q, j] = i, -s
        if tg is not None:
            for t, item in enumerate(tg):
                if mask_profile and item in S[u]:
                    continue
                rank[q, t] = cand.index((-acc.get(item, 0), item))     # the sorted list holds every candidate once: its position is what beats it
    return idx, score, rank


def lists_of(interact, k, measure='cosine', shrink=0.0):
    """(nbr_idx, nbr_w) of the user side of `interact` from the restated cooccur_topk and the weights formed element by element."""
    import cooccur_restatement as C
    idx, cnt, deg = C.cooccur_topk(sp.csr_matrix(interact), k, measure)
    w = np.zeros(idx.shape, np.int32)
    for u in range(idx.shape[0]):
        for r in range(idx.shape[1]):
            v, c = int(idx[u, r]), int(cnt[u, r])
            if v < 0:
                continue
            if measure == 'count':
                w[u, r] = c
            elif measure == 'cosine':
                w[u, r] = int(np.floor(c / (np.sqrt(np.float64(int(deg[u]) * int(deg[v]))) + shrink) * 2 ** 30))
            else:
                w[u, r] = int(np.floor(c / (np.float64(int(deg[u]) + int(deg[v]) - c) + shrink) * 2 ** 30))
    return idx, w


def small(seed=11, U=60, I=150):
    """The planted input of the user-kNN GPU tests, built for the cursor walk at tile sizes 16 and 64.  60 users x 150 items:
      rows 0..39  random, 3..25 items;
      row 40      empty;                       row 41  the whole catalogue;
      row 42      {15, 16}: entries at t1 - 1 and t1 of tile 16;
      row 43      {0..15}: ends exactly at a tile's end;
      row 44      {2, 3, 100, 140}: no entry in the middle tiles;
      rows 45..48 row segments of 63, 64, 65 and 128 entries (inside one tile at the default tile; chunk seams of the 64-lane walk);
      rows 49..51 identical rows {1, 5, 8};
      rows 52..59 fake rows: the targets {140, 141, 149} and the popular items {0..5}."""
    rng = np.random.RandomState(seed)
    D = np.zeros((U, I), np.int64)
    for u in range(40):
        D[u, rng.choice(I, rng.randint(3, 26), replace=False)] = 1
    D[41] = 1
    D[42, [15, 16]] = 1
    D[43, :16] = 1
    D[44, [2, 3, 100, 140]] = 1
    for u, n in zip(range(45, 49), (63, 64, 65, 128)):
        D[u, 7:7 + n] = 1
    D[49:52, [1, 5, 8]] = 1
    D[52:, [140, 141, 149]] = 1
    D[52:, :6] = 1
    return sp.csr_matrix(D)

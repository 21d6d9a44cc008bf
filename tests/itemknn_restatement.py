"""The contract of arlib_amd.itemknn.knn_score_topk restated in pure Python: a dict accumulator of Python ints per user, a sort on
(-score, id) tuples, the target ranks counted one candidate at a time.  Slow on purpose and free of numpy arithmetic, so that it shares nothing
with the kernel or the host route.  The inputs come from tests/cooccur_restatement.py (planted(), identical_rows())."""
import numpy as np
import scipy.sparse as sp

from cooccur_restatement import sets_of, planted, identical_rows  # noqa: F401  (re-exported for the tests)


def knn_score_topk(interact, nbr_idx, nbr_w, N, rows=None, mask_profile=False, targets=None):
    S = sets_of(interact)
    n_items = sp.csr_matrix(interact).shape[1]
    ni, nw = np.asarray(nbr_idx).tolist(), np.asarray(nbr_w).tolist()
    queries = list(range(len(S))) if rows is None else [int(r) for r in rows]
    tg = None if targets is None else [int(t) for t in targets]
    idx, score = np.full((len(queries), N), -1, np.int32), np.zeros((len(queries), N), np.int64)
    rank = None if tg is None else np.full((len(queries), len(tg)), -1, np.int32)
    for q, u in enumerate(queries):
        acc = {}
        for j in S[u]:
            for i, w in zip(ni[j], nw[j]):
                if i >= 0:
                    acc[i] = acc.get(i, 0) + int(w)
        cand = [(-acc.get(i, 0), i) for i in range(n_items) if not (mask_profile and i in S[u])]
        cand.sort()
        for j, (s, i) in enumerate(cand[:N]):
            idx[q, j], score[q, j] = i, -s
        if tg is not None:
            for t, item in enumerate(tg):
                if mask_profile and item in S[u]:
                    continue
                key = (-acc.get(item, 0), item)
                rank[q, t] = cand.index(key)                # the sorted list holds every candidate once: its position is what beats it
    return idx, score, rank


def lists_of(interact, k, measure='cosine', shrink=0.0):
    """(nbr_idx, nbr_w) of the item side of `interact` from the restated cooccur_topk and the weights formed element by element."""
    import cooccur_restatement as C
    XT = sp.csr_matrix(sp.csr_matrix(interact).T)
    idx, cnt, deg = C.cooccur_topk(XT, k, measure)
    w = np.zeros(idx.shape, np.int32)
    for j in range(idx.shape[0]):
        for r in range(idx.shape[1]):
            v, c = int(idx[j, r]), int(cnt[j, r])
            if v < 0:
                continue
            if measure == 'count':
                w[j, r] = c
            elif measure == 'cosine':
                w[j, r] = int(np.floor(c / (np.sqrt(np.float64(int(deg[j]) * int(deg[v]))) + shrink) * 2 ** 30))
            else:
                w[j, r] = int(np.floor(c / (np.float64(int(deg[j]) + int(deg[v]) - c) + shrink) * 2 ** 30))
    return idx, w

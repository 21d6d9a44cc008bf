"""The contract of arlib_amd.neighbours.cooccur_topk restated in pure Python: dense counts, keys of Python ints, a comparison sort with the id as
tie-break.  Slow on purpose and free of numpy arithmetic in the ordering, so that it shares nothing with the kernel or the host route."""
import functools

import numpy as np
import scipy.sparse as sp


def sets_of(interact):
    X = sp.csr_matrix(interact)
    return [set(int(c) for c, x in zip(X.indices[X.indptr[r]:X.indptr[r + 1]], X.data[X.indptr[r]:X.indptr[r + 1]]) if x != 0) for r in range(X.shape[0])]


def before(measure, du):
    def cmp(a, b):                                          # a, b = (c, d, id)
        if measure == 'count':
            ka, kb = a[0], b[0]
        elif measure == 'cosine':
            ka, kb = a[0] * a[0] * b[1], b[0] * b[0] * a[1]
        elif measure == 'jaccard':
            ka, kb = a[0] * (du + b[1] - b[0]), b[0] * (du + a[1] - a[0])
        else:
            raise ValueError(measure)
        if ka != kb:
            return -1 if ka > kb else 1
        return -1 if a[2] < b[2] else (1 if a[2] > b[2] else 0)
    return cmp


def cooccur_topk(interact, k, measure='cosine', rows=None):
    S = sets_of(interact)
    n = len(S)
    deg = [len(s) for s in S]
    queries = list(range(n)) if rows is None else [int(r) for r in rows]
    idx, cnt = np.full((len(queries), k), -1, np.int32), np.zeros((len(queries), k), np.int32)
    for q, u in enumerate(queries):
        cand = [(len(S[u] & S[v]), deg[v], v) for v in range(n) if v != u and S[u] & S[v]]
        cand.sort(key=functools.cmp_to_key(before(measure, deg[u])))
        for j, (c, _, v) in enumerate(cand[:k]):
            idx[q, j], cnt[q, j] = v, c
    return idx, cnt, np.asarray(deg, np.int64)


def similarity(idx, cnt, deg, rows, measure):
    """float64 similarities from the integers, element by element."""
    out = np.zeros(idx.shape, np.float64)
    for q in range(idx.shape[0]):
        u = q if rows is None else int(rows[q])
        for j in range(idx.shape[1]):
            v, c = int(idx[q, j]), int(cnt[q, j])
            if v >= 0:
                out[q, j] = c if measure == 'count' else (c / np.sqrt(np.float64(int(deg[u]) * int(deg[v]))) if measure == 'cosine' else c / np.float64(int(deg[u]) + int(deg[v]) - c))
    return out


def planted(seed=7, U=300, F=20, I=400):
    """The planted input of the detection tests: U real rows of randint(5, 40) distinct items drawn with p ~ (1 + i)^-0.8, then F fake rows of the
    targets {390, 391, 392}, the popular items {0..11} and 10 uniform distinct items.  Returns (csr int64 [U + F, I], fake ids)."""
    rng = np.random.RandomState(seed)
    p = (1.0 + np.arange(I)) ** -0.8
    p /= p.sum()
    D = np.zeros((U + F, I), np.int64)
    for u in range(U):
        D[u, rng.choice(I, rng.randint(5, 40), replace=False, p=p)] = 1
    for f in range(F):
        D[U + f, [390, 391, 392]] = 1
        D[U + f, :12] = 1
        D[U + f, rng.choice(I, 10, replace=False)] = 1
    return sp.csr_matrix(D), np.arange(U, U + F)


def identical_rows(n=150, I=40):
    """Every row the same set: every similarity ties, so the neighbours of u are the smallest ids other than u."""
    D = np.zeros((n, I), np.int64)
    D[:, [1, 5, 8, 13, 21, 34]] = 1
    return sp.csr_matrix(D)

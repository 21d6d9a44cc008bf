"""Fake-user detection on the exact top-k profile neighbours of arlib_amd/neighbours.py (no reference counterpart).  The
classical unsupervised profile features on implicit feedback -- DegSim (Chirita et al. 2005), the in-degree in the kNN graph, Burke's LengthVar
and the mean popularity of a profile's items -- a detector on the first of them, and `sanitize`, which drops the top-scored profiles so that a
victim can be retrained on what is left.  The neighbour lists are integers, the float64 features are formed from them on the host, so the
features do not depend on whether the lists came from the kernel or from the host route."""
import numpy as np
import scipy.sparse as sp

from .. import neighbours


def profile_features(interact, k=25, measure='cosine', device=None):
    """dict of float64 arrays [U] for the U x I interaction matrix (any nonzero entry counts as 1):
      degsim           the mean similarity to the k nearest other users, a missing neighbour counting as 0;
      knn_indegree     the number of users that list this user among their k neighbours;
      length_var       Burke's LengthVar, |n_u - mean n| / sum_v (n_v - mean n)^2 (0 when every profile has the same length);
      mean_popularity  the mean over the profile's items of (item degree / U), 0 for an empty profile.
    device None takes the host route of the neighbour search (scipy), anything else neighbours.cooccur_topk(route='auto') on that device."""
    X = neighbours.binary_csr(interact)
    U = X.shape[0]
    if device is None:
        idx, cnt, deg = neighbours.cooccur_topk_host(X, k, measure)
    else:
        idx, cnt, deg = neighbours.cooccur_topk(X.indptr, X.indices, U, X.shape[1], k, measure, device=device)
        idx, cnt, deg = idx.cpu().numpy(), cnt.cpu().numpy(), deg.cpu().numpy()
    sim = neighbours.similarity(idx, cnt, deg, None, measure)
    n = deg.astype(np.float64)
    dev2 = ((n - n.mean()) ** 2).sum() if U else 0.0
    pop = np.asarray(X.sum(0), dtype=np.float64).ravel() / max(U, 1)
    return {'degsim': sim.sum(1) / float(k),
            'knn_indegree': np.bincount(idx[idx >= 0].astype(np.int64), minlength=U).astype(np.float64),
            'length_var': np.abs(n - n.mean()) / dev2 if dev2 > 0 else np.zeros(U),
            'mean_popularity': np.asarray(X @ pop, dtype=np.float64).ravel() / np.maximum(n, 1.0)}


class DegSimDetector(object):
    """Scores a user by DegSim: a block of injected profiles built by one rule is far more self-similar than real users are to their neighbours,
    so higher = more suspicious."""

    def __init__(self, k=25, measure='cosine', device=None):
        self.k, self.measure, self.device = int(k), measure, device

    def score(self, interact):
        return profile_features(interact, self.k, self.measure, self.device)['degsim']

    def flag(self, interact, n):
        """The ids of the n most suspicious users, most suspicious first, ties to the smaller id."""
        s = self.score(interact)
        return np.lexsort((np.arange(len(s)), -s))[:int(n)]


def sanitize(interact, scores, n_drop):
    """(kept, reduced): the ascending row ids that remain after the n_drop top-scored rows (ties to the smaller id) are dropped, and the CSR
    matrix of those rows with the columns unchanged, ready for DataLoader.from_arrays / ArrayDataLoader through its (row, col, value) triplets."""
    X = sp.csr_matrix(interact)
    s = np.asarray(scores, dtype=np.float64).ravel()
    n_drop = int(n_drop)
    if len(s) != X.shape[0] or not 0 <= n_drop <= len(s):
        raise ValueError('sanitize: %d scores for %d rows, n_drop = %d' % (len(s), X.shape[0], n_drop))
    drop = np.lexsort((np.arange(len(s)), -s))[:n_drop]
    keep = np.ones(len(s), bool)
    keep[drop] = False
    kept = np.flatnonzero(keep)
    return kept, X[kept]

"""Ranking metrics with the reference's interface and output format (util/metrics.py:87-114 ranking_evaluation,
:125-208 AttackMetric).  Host-side bookkeeping around the top-k lists the GPU produces; AttackMetric replaces the
reference's per-user predict()+argsort loop by one streaming score+top-k kernel launch over all users.
"""
import math

import numpy as np


class RecommendMetric(object):
    @staticmethod
    def hits(origin, res):
        return {u: len(set(origin[u]).intersection(i[0] for i in res[u])) for u in origin}

    @staticmethod
    def hit_ratio(origin, hits):
        total = sum(len(origin[u]) for u in origin)
        return sum(hits.values()) / total

    @staticmethod
    def precision(hits, N):
        return sum(hits.values()) / (len(hits) * N)

    @staticmethod
    def recall(hits, origin):
        vals = [hits[u] / len(origin[u]) for u in hits]
        return sum(vals) / len(vals)

    @staticmethod
    def F1(prec, recall):
        return 2 * prec * recall / (prec + recall) if (prec + recall) != 0 else 0

    @staticmethod
    def NDCG(origin, res, N):
        total = 0
        for user in res:
            dcg = sum(1.0 / math.log(n + 2) for n, item in enumerate(res[user]) if item[0] in origin[user])
            idcg = sum(1.0 / math.log(n + 2) for n in range(min(len(origin[user]), N)))
            total += dcg / idcg
        return total / len(res)


def ranking_evaluation(origin, res, N):
    measure = []
    for n in N:
        predicted = {user: res[user][:n] for user in res}
        if len(origin) != len(predicted):
            print('The Lengths of test set and predicted set do not match!')
            exit(-1)
        hits = RecommendMetric.hits(origin, predicted)
        measure.append('Top ' + str(n) + '\n')
        measure.append('Hit Ratio:' + str(RecommendMetric.hit_ratio(origin, hits)) + '\n')
        measure.append('Precision:' + str(RecommendMetric.precision(hits, n)) + '\n')
        measure.append('Recall:' + str(RecommendMetric.recall(hits, origin)) + '\n')
        measure.append('NDCG:' + str(RecommendMetric.NDCG(origin, predicted, n)) + '\n')
    return measure


def test_set_image(data):
    """Per test user (in test_set order): how many test items it has, and the (row, internal item id) keys of those the model
    knows, sorted -- built once per data object (the test split never changes)."""
    img = getattr(data, '_arl_test_image', None)
    if img is None or img[0] != len(data.test_set):
        users = list(data.test_set)
        lens = np.array([len(data.test_set[u]) for u in users], np.int64)
        I = len(data.item)
        keys = np.array(sorted(r * I + data.item[it] for r, u in enumerate(users) for it in data.test_set[u] if it in data.item), np.int64)
        img = (len(users), users, lens, keys)
        data._arl_test_image = img
    return img


def ranking_evaluation_topk(data, idx, N):
    """The measure lines of ranking_evaluation(data.test_set, rec_list, N) computed from the top-k index array idx
    [test users in test_set order, >= max(N)] without building rec_list.  Same arithmetic in the same order (integer hit
    counts; rank-ordered DCG terms; the user-ordered Python float accumulations), hence the same strings."""
    _, users, lens, keys = test_set_image(data)
    I = len(data.item)
    idx = np.asarray(idx, np.int64)
    pk = np.arange(idx.shape[0], dtype=np.int64)[:, None] * I + idx
    pos = np.searchsorted(keys, pk)
    H = keys[np.minimum(pos, max(len(keys) - 1, 0))] == pk if len(keys) else np.zeros(pk.shape, bool)
    total = int(lens.sum())
    measure = []
    for n in N:
        Hn = H[:, :n]
        hits = Hn.sum(1).astype(np.int64)
        s_hits = int(hits.sum())
        w = [1.0 / math.log(r + 2) for r in range(n)]
        dcg = np.zeros(idx.shape[0], np.float64)
        for r in range(min(n, Hn.shape[1])):
            dcg = dcg + np.where(Hn[:, r], w[r], 0.0)
        pref = [0]
        for r in range(n):
            pref.append(pref[-1] + w[r])
        idcg = np.array([pref[m] for m in np.minimum(lens, n).tolist()], np.float64)
        ndcg_total = 0
        for v in (dcg / idcg).tolist():
            ndcg_total += v
        measure.append('Top ' + str(n) + '\n')
        measure.append('Hit Ratio:' + str(s_hits / total) + '\n')
        measure.append('Precision:' + str(s_hits / (len(hits) * n)) + '\n')
        measure.append('Recall:' + str(sum((hits / lens).tolist()) / len(hits)) + '\n')
        measure.append('NDCG:' + str(ndcg_total / len(hits)) + '\n')
    return measure


class AttackMetric(object):
    """targetItem: internal item ids.  Rankings are over ALL items without masking interacted ones, as in the
    reference (np.argsort(-score)[:k], util/metrics.py:141)."""

    def __init__(self, recommendModel, targetItem, top=[10]):
        self.recommendModel = recommendModel
        self.targetItem = targetItem
        self.top = top
        self._rank = None

    def _top(self):
        if self._rank is None:
            import torch
            from .. import ops
            rm = self.recommendModel
            if hasattr(rm, 'topk_all_users'):                 # a model without embedding tables ranks for itself (recommender/ItemKNN.py)
                self._rank = np.asarray(rm.topk_all_users(max(self.top)))
                return self._rank
            uid = torch.tensor([rm.data.user[u] for u in rm.data.user], dtype=torch.long, device=rm.user_emb.device)
            Pu, Pi = rm.user_emb[uid].contiguous(), rm.item_emb.contiguous()
            k = min(max(self.top), Pi.shape[0])
            if Pu.shape[1] % 4 == 0 and k <= 128:
                idx, _ = ops.score_mask_topk(Pu, Pi, k)
            else:
                idx = torch.topk(Pu @ Pi.T, k)[1]
            self._rank = idx.cpu().numpy()
        return self._rank

    def _hits(self):
        """hit[u, r] = True when the r-th ranked item of user u is a target."""
        return np.isin(self._top(), np.asarray(self.targetItem))

    def precision(self):
        h = self._hits()
        return [float(h[:, :k].sum() / (h.shape[0] * k)) for k in self.top]

    def hitRate(self):
        h = self._hits()
        return [float((h[:, :k].any(1) / len(self.targetItem)).sum() / h.shape[0]) for k in self.top]

    def recall(self):
        h = self._hits()
        return [float(h[:, :k].sum() / (h.shape[0] * len(self.targetItem))) for k in self.top]

    def NDCG(self):
        h = self._hits()
        out = []
        for k in self.top:
            disc = 1.0 / np.log2(2 + np.arange(k))
            idcg = disc[:min(k, len(self.targetItem))].sum()
            out.append(float((h[:, :k] * disc).sum() / (idcg * h.shape[0])))
        return out


class TargetRankMetric(object):
    """Full-ranking attack metrics: the rank of every target item for every user over the whole catalogue (ops.target_rank, one call), and everything
    that follows from it.  targetItem: internal item ids (distinct).  top: any k up to the number of items.  mask_train=True leaves each user's training
    interactions out of the ranking; a pair whose target the user already has gets rank -1 and drops out of every count below, while the user-level
    denominators of the four reference formulas stay as they are.

    hitRate / precision / recall / NDCG are AttackMetric's formulas (reference util/metrics.py:125-208) with hit[u, r] read as "some target of user u has
    rank r": they depend on `rank < k` and `disc[rank]` only, so the rank matrix serves them at every k without a top-k list."""

    def __init__(self, recommendModel, targetItem, top=[10], mask_train=False):
        self.recommendModel = recommendModel
        self.targetItem = targetItem
        self.top = top
        self.mask_train = mask_train
        self._rank = None

    def ranks(self):
        """int32 [U, T]: 0-based rank of target t in user u's descending score row (ties by item id), -1 where the pair is masked."""
        if self._rank is None:
            import torch
            from .. import ops
            rm = self.recommendModel
            if hasattr(rm, 'target_ranks'):                   # likewise
                self._rank = np.asarray(rm.target_ranks(self.targetItem, mask_train=self.mask_train))
                return self._rank
            dev = rm.user_emb.device
            ids = [rm.data.user[u] for u in rm.data.user]
            uid = torch.tensor(ids, dtype=torch.long, device=dev)
            Pu, Pi = rm.user_emb[uid].detach().float().contiguous(), rm.item_emb.detach().float().contiguous()
            targets = torch.tensor([int(t) for t in self.targetItem], dtype=torch.int32, device=dev)
            mask = None
            if self.mask_train:
                m = rm.data.matrix().tocsr()[np.asarray(ids, np.int64)]
                m.sum_duplicates()
                m.sort_indices()
                mask = (torch.from_numpy(m.indptr.astype(np.int32)).to(dev), torch.from_numpy(m.indices.astype(np.int32)).to(dev))
            rank, _ = ops.target_rank(Pu, Pi, targets, mask)
            self._rank = rank.cpu().numpy()
        return self._rank

    def _below(self, k):
        r = self.ranks()
        return (r >= 0) & (r < k)

    def precision(self):
        r = self.ranks()
        return [float(self._below(k).sum() / (r.shape[0] * k)) for k in self.top]

    def hitRate(self):
        r = self.ranks()
        return [float((self._below(k).any(1) / r.shape[1]).sum() / r.shape[0]) for k in self.top]

    def recall(self):
        r = self.ranks()
        return [float(self._below(k).sum() / (r.shape[0] * r.shape[1])) for k in self.top]

    def NDCG(self):
        r = self.ranks()
        out = []
        for k in self.top:
            disc = 1.0 / np.log2(2 + np.arange(k))
            idcg = disc[:min(k, r.shape[1])].sum()
            b = self._below(k)
            out.append(float(disc[r[b]].sum() / (idcg * r.shape[0])))
        return out

    def meanRank(self):
        """Mean over the valid pairs of the 1-based rank."""
        r = self.ranks()
        v = r >= 0
        return float((r[v].astype(np.float64) + 1.0).mean()) if v.any() else float('nan')

    def MRR(self):
        """Mean over the valid pairs of 1 / (1-based rank)."""
        r = self.ranks()
        v = r >= 0
        return float((1.0 / (r[v].astype(np.float64) + 1.0)).mean()) if v.any() else float('nan')

    def exposure(self, per_target=False):
        """ER@K for each K of `top`: per target, the share of its valid pairs with rank < K; averaged over the targets that have a valid pair
        (per_target=True: the [T] array itself, NaN for a target without one)."""
        r = self.ranks()
        valid = (r >= 0).sum(0).astype(np.float64)
        out = []
        for k in self.top:
            with np.errstate(invalid='ignore', divide='ignore'):
                share = self._below(k).sum(0) / valid
            out.append(share if per_target else (float(np.nanmean(share)) if (valid > 0).any() else float('nan')))
        return out


class DetectionMetric(object):
    """How well per-user suspicion scores separate injected profiles from real ones (no reference counterpart).  scores [n]: higher = more
    suspicious; fake_ids: the ids of the injected users (distinct, in [0, n)).  The ranking behind the @n figures is by descending score, ties
    to the smaller id, so every figure is a function of the scores alone."""

    def __init__(self, scores, fake_ids):
        self.scores = np.asarray(scores, dtype=np.float64).ravel()
        fake = np.asarray(fake_ids, dtype=np.int64).ravel()
        n = len(self.scores)
        if np.isnan(self.scores).any():
            raise ValueError('DetectionMetric: NaN score')
        if len(fake) and (fake.min() < 0 or fake.max() >= n or len(np.unique(fake)) != len(fake)):
            raise ValueError('DetectionMetric: fake_ids must be distinct ids in [0, %d)' % n)
        self.is_fake = np.zeros(n, bool)
        self.is_fake[fake] = True
        self._order = np.lexsort((np.arange(n), -self.scores))

    def auc(self):
        """Mann-Whitney: the share of (fake, real) pairs in which the fake user scores higher, a tied pair counting one half (average ranks).
        Counted in integers and divided once; NaN without a fake or without a real user."""
        pos, neg = np.sort(self.scores[self.is_fake]), np.sort(self.scores[~self.is_fake])
        if len(pos) == 0 or len(neg) == 0:
            return float('nan')
        below = np.searchsorted(neg, pos, side='left').astype(np.int64)
        tied = np.searchsorted(neg, pos, side='right').astype(np.int64) - below
        return float(int(2 * below.sum() + tied.sum()) / (2 * len(pos) * len(neg)))

    def _hits(self, n):
        n = int(n)
        if n < 1:
            raise ValueError('DetectionMetric: n = %d, n >= 1 needed' % n)
        return int(self.is_fake[self._order[:n]].sum()), min(n, len(self.scores))

    def precision_at(self, n):
        h, m = self._hits(n)
        return h / m if m else float('nan')

    def recall_at(self, n):
        h, _ = self._hits(n)
        f = int(self.is_fake.sum())
        return h / f if f else float('nan')

    def f1_at(self, n):
        p, r = self.precision_at(n), self.recall_at(n)
        return 2 * p * r / (p + r) if p + r > 0 else 0.0

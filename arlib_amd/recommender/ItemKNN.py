"""ItemKNN: item-based top-N recommendation (Deshpande & Karypis, TOIS'04) -- the neighbourhood recommender the shilling attacks (Random,
Bandwagon, AUSH, GOAT, LegUP) were published against.  The reference ships no such model; like iALS it is an addition with the Recommender
surface, so posionDataAttack() output -> ItemKNN(args, data).train() -> AttackMetric / TargetRankMetric / test() closes the loop for that family.

    s(u, i) = sum over j in P_u of sim(j, i) [i among the knn_k nearest neighbours of j]

The item-side lists are neighbours.cooccur_topk on the transposed training matrix (integers), the weights itemknn.knn_weights (fixed point,
floor(sim 2^30); 'count': the co-occurrence count), the scores and lists itemknn.knn_score_topk (exact int64 sums, order (score descending, item
id ascending)); floats are formed from those integers in one place (itemknn.float_score), so a GPU run and a host run agree bit for bit
(DESIGN.md section 3t).  There are no embedding tables, no epochs, no sampler and no optimizer: train() builds the lists once, and nothing is
drawn from `random` or torch's generator."""
import sys

import numpy as np
import scipy.sparse as sp
import torch

from .. import itemknn, neighbours
from ..util.metrics import ranking_evaluation, ranking_evaluation_topk
from ._base import Recommender


class ItemKNN(Recommender):
    knn_k = 50                        # neighbours kept per item; args.knn_k overrides
    knn_measure = 'cosine'            # 'count', 'cosine' or 'jaccard'; args.knn_measure overrides
    knn_shrink = 0.0                  # added to the similarity's denominator; args.knn_shrink overrides
    knn_route = 'auto'                # the route of cooccur_topk and knn_score_topk: 'auto', 'kernel' or 'host'; args.knn_route overrides

    def __init__(self, args, data):
        self._common_init(args, data, 'ItemKNN')
        for k, conv in (('knn_k', int), ('knn_measure', str), ('knn_shrink', float), ('knn_route', str)):
            setattr(self, k, conv(getattr(args, k, getattr(type(self), k))))
        if self.knn_k < 1 or self.knn_measure not in neighbours.MEASURES or not self.knn_shrink >= 0.0 or self.knn_route not in itemknn.ROUTES:
            raise ValueError("ItemKNN: knn_k >= 1, knn_measure in ('count', 'cosine', 'jaccard'), knn_shrink >= 0 and knn_route in ('auto', 'kernel', 'host')")
        self.device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.nbr_idx = self.nbr_cnt = self.nbr_w = self.item_deg = None
        self._X = self._W = self._dev_lists = None

    # ---- the model: the training matrix and the item-side lists
    def _matrix(self):
        return neighbours.binary_csr(self.data.interaction_mat)

    def fit(self):
        """The item-side neighbour lists of the current training matrix: (nbr_idx, nbr_cnt int32 [I, knn_k], item_deg int64 [I]) and nbr_w."""
        X = self._matrix()
        XT = sp.csr_matrix(X.T)
        XT.sort_indices()
        I, U = XT.shape
        idx, cnt, deg = neighbours.cooccur_topk(XT.indptr.astype(np.int64), XT.indices.astype(np.int32), I, U, self.knn_k, self.knn_measure,
                                                device=self.device, route=self.knn_route)
        self.nbr_idx, self.nbr_cnt, self.item_deg = idx.cpu().numpy(), cnt.cpu().numpy(), deg.cpu().numpy()
        self.nbr_w = itemknn.knn_weights(self.nbr_idx, self.nbr_cnt, self.item_deg, self.knn_measure, self.knn_shrink)
        self._X, self._W = X, None
        self._dev_lists = None

    def _fitted(self):
        if self.nbr_idx is None:
            raise RuntimeError('ItemKNN: train() first')

    def _score_topk(self, rows, N, mask, targets=None):
        """knn_score_topk on the fitted lists, as numpy arrays."""
        self._fitted()
        X = self._X
        if self._dev_lists is None:                               # the lists travel to the device once
            dev = self.device if self.knn_route != 'host' else 'cpu'
            self._dev_lists = tuple(torch.from_numpy(a).to(dev) for a in (X.indptr.astype(np.int64), X.indices.astype(np.int32), self.nbr_idx, self.nbr_w))
        rp, ci, ni, nw = self._dev_lists
        idx, score, rank = itemknn.knn_score_topk(rp, ci, X.shape[0], X.shape[1], ni, nw, N, rows=None if rows is None else np.asarray(rows, np.int64),
                                                  mask_profile=mask, targets=targets, device=self.device, route=self.knn_route)
        return idx.cpu().numpy(), score.cpu().numpy(), None if rank is None else rank.cpu().numpy()

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5, requires_grad=False):
        if requires_grad:
            raise NotImplementedError('requires_grad is not implemented for ItemKNN: its lists are counted, no gradient step is taken')
        if requires_embgrad:
            raise NotImplementedError('requires_embgrad is not implemented for ItemKNN: the model has no embedding tables')
        if requires_adjgrad:
            raise NotImplementedError('requires_adjgrad is not implemented for ItemKNN: the model has no adjacency')
        self.bestPerformance = []
        self.fit()
        print('training: neighbour lists of', self.nbr_idx.shape[0], 'items, k =', self.knn_k, 'measure:', self.knn_measure)
        self.evaluate(0)

    def save(self):
        pass                                                      # one fit, nothing to keep beside it

    # ---- evaluation
    def _test_topk(self):
        """(test users in test_set order, top-max_N item ids [n, k] with -1 past the candidates, float scores) with the training items masked."""
        users = list(self.data.test_set)
        if not users:
            return users, np.zeros((0, 0), np.int64), np.zeros((0, 0), np.float64)
        idx, score, _ = self._score_topk([self.data.user[u] for u in users], min(self.max_N, len(self.data.item)), True)
        return users, idx.astype(np.int64), itemknn.float_score(score, self.knn_measure)

    def _rec_list(self, users, idx, val):
        return {user: [(self.data.id2item[int(i)], float(s)) for i, s in zip(idx[r], val[r]) if i >= 0] for r, user in enumerate(users)}

    def _measures(self, users, idx, val, Ns):
        if users and bool((idx >= 0).all()):
            return ranking_evaluation_topk(self.data, idx, Ns)
        return ranking_evaluation(self.data.test_set, self._rec_list(users, idx, val), Ns)     # a user with fewer candidates than N: the plain form

    def evaluate(self, epoch):
        print('Evaluating the model...')
        users, idx, val = self._test_topk()
        sys.stdout.write('\rProgress: [' + '+' * 50 + ']100%\n')
        measure = self._measures(users, idx, val, [self.max_N])
        performance = {}
        for m in measure[1:]:
            k, v = m.strip().split(':')
            performance[k] = float(v)
        self.bestPerformance = [epoch + 1, performance]
        print('-' * 120)
        print('Real-Time Ranking Performance ' + ' (Top-' + str(self.max_N) + ' Item Recommendation)')
        measure = [m.strip() for m in measure[1:]]
        print('*Current Performance*')
        print('Epoch:', str(epoch + 1) + ',', '  |  '.join(measure))
        print('-' * 120)
        return measure

    def test(self):
        users, idx, val = self._test_topk()
        rec_list = self._rec_list(users, idx, val)
        sys.stdout.write('\rProgress: [' + '+' * 50 + ']100%\n')
        return rec_list, self._measures(users, idx, val, self.topN)

    def predict(self, u):
        """The dense float score row of user u (a raw id) over the whole catalogue."""
        self._fitted()
        if self._W is None:
            self._W = itemknn.weight_matrix(self.nbr_idx, self.nbr_w, self._X.shape[1])
        row = np.asarray((self._X[self.data.get_user_id(u)] @ self._W).todense(), dtype=np.int64).ravel()
        return itemknn.float_score(row, self.knn_measure)

    # ---- the hooks util.metrics.AttackMetric / TargetRankMetric look for
    def _all_users(self):
        return [self.data.user[u] for u in self.data.user]

    def topk_all_users(self, k, mask_train=False):
        """int64 [U, min(k, I)]: the k best items of every user of data.user, in that order; -1 past the candidates."""
        return self._score_topk(self._all_users(), min(int(k), len(self.data.item)), bool(mask_train))[0].astype(np.int64)

    def target_ranks(self, targets, mask_train=False):
        """int32 [U, T]: the 0-based rank of every target (internal item ids, distinct) for every user of data.user, -1 where masked."""
        tg = np.asarray([int(t) for t in targets], np.int64)
        return self._score_topk(self._all_users(), 1, bool(mask_train), tg)[2]

    def neighbours_of(self, item):
        """[(raw item id, float similarity)] of the fitted list of `item` (a raw id), best first."""
        self._fitted()
        j = self.data.get_item_id(item)
        sim = itemknn.knn_similarity(self.nbr_idx, self.nbr_cnt, self.item_deg, self.knn_measure, self.knn_shrink)[j]
        return [(self.data.id2item[int(v)], float(s)) for v, s in zip(self.nbr_idx[j], sim) if v >= 0]

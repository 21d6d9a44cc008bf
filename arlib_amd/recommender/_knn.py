"""What the neighbourhood recommenders (ItemKNN, UserKNN) share: the training matrix, the evaluation surface of the Recommender classes
(_test_topk, _rec_list, _measures, evaluate, test, save) and the hooks util.metrics.AttackMetric / TargetRankMetric look for (topk_all_users,
target_ranks), all on one method of the subclass, _score_topk(rows, N, mask, targets) -> numpy (idx int32, score int64, rank int32 or None),
and on itemknn.float_score for the floats.  A subclass sets nbr_idx in fit() and knn_measure in __init__."""
import sys

import numpy as np

from .. import itemknn, neighbours
from ..util.metrics import ranking_evaluation, ranking_evaluation_topk
from ._base import Recommender


class KNNRecommender(Recommender):
    def _matrix(self):
        return neighbours.binary_csr(self.data.interaction_mat)

    def _fitted(self):
        if self.nbr_idx is None:
            raise RuntimeError('%s: train() first' % type(self).__name__)

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

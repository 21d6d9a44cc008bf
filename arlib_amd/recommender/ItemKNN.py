"""ItemKNN: item-based top-N recommendation (Deshpande & Karypis, TOIS'04) -- the neighbourhood recommender the shilling attacks (Random,
Bandwagon, AUSH, GOAT, LegUP) were published against.  The reference ships no such model; like iALS it is an addition with the Recommender
surface, so posionDataAttack() output -> ItemKNN(args, data).train() -> AttackMetric / TargetRankMetric / test() closes the loop for that family.

    s(u, i) = sum over j in P_u of sim(j, i) [i among the knn_k nearest neighbours of j]

The item-side lists are neighbours.cooccur_topk on the transposed training matrix (integers), the weights itemknn.knn_weights (fixed point,
floor(sim 2^30); 'count': the co-occurrence count), the scores and lists itemknn.knn_score_topk (exact int64 sums, order (score descending, item
id ascending)); floats are formed from those integers in one place (itemknn.float_score), so a GPU run and a host run agree bit for bit
(DESIGN.md section 3t).  There are no embedding tables, no epochs, no sampler and no optimizer: train() builds the lists once, and nothing is
drawn from `random` or torch's generator."""
import numpy as np
import scipy.sparse as sp
import torch

from .. import itemknn, neighbours
from ._knn import KNNRecommender


class ItemKNN(KNNRecommender):
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

    # ---- the model: the item-side lists of the training matrix
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

    # ---- evaluation: KNNRecommender's, on _score_topk above
    def predict(self, u):
        """The dense float score row of user u (a raw id) over the whole catalogue."""
        self._fitted()
        if self._W is None:
            self._W = itemknn.weight_matrix(self.nbr_idx, self.nbr_w, self._X.shape[1])
        row = np.asarray((self._X[self.data.get_user_id(u)] @ self._W).todense(), dtype=np.int64).ravel()
        return itemknn.float_score(row, self.knn_measure)

    def neighbours_of(self, item):
        """[(raw item id, float similarity)] of the fitted list of `item` (a raw id), best first."""
        self._fitted()
        j = self.data.get_item_id(item)
        sim = itemknn.knn_similarity(self.nbr_idx, self.nbr_cnt, self.item_deg, self.knn_measure, self.knn_shrink)[j]
        return [(self.data.id2item[int(v)], float(s)) for v, s in zip(self.nbr_idx[j], sim) if v >= 0]

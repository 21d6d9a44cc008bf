"""UserKNN: user-based top-N recommendation (Resnick et al., CSCW'94; Herlocker et al., SIGIR'99) -- the recommender the shilling literature
started from (Lam & Riedl, WWW'04; Mobasher et al., TOIT'07): a fake profile acts by entering the neighbourhoods of real users.  The reference
ships no such model; like ItemKNN it is an addition with the Recommender surface, so posionDataAttack() output -> UserKNN(args, data).train() ->
AttackMetric / TargetRankMetric / test() closes the loop for that family.

    s(u, i) = sum over the knn_k nearest neighbours v of u of sim(u, v) [i in P_v]

The user-side lists are neighbours.cooccur_topk on the training matrix itself (integers) -- the lists detect.profile_features counts knn_indegree
on -- the weights itemknn.knn_weights (fixed point, floor(sim 2^30); 'count': the co-occurrence count), the scores and lists
userknn.uknn_score_topk (exact int64 sums, order (score descending, item id ascending)); floats are formed from those integers in one place
(itemknn.float_score), so a GPU run and a host run agree bit for bit.  There are no embedding tables, no epochs, no
sampler and no optimizer: train() builds the lists once, and nothing is drawn from `random` or torch's generator."""
import numpy as np
import torch

from .. import itemknn, neighbours, userknn
from ._knn import KNNRecommender


class UserKNN(KNNRecommender):
    knn_k = 50                        # neighbours kept per user; args.knn_k overrides
    knn_measure = 'cosine'            # 'count', 'cosine' or 'jaccard'; args.knn_measure overrides
    knn_shrink = 0.0                  # added to the similarity's denominator; args.knn_shrink overrides
    knn_route = 'auto'                # the route of cooccur_topk and uknn_score_topk: 'auto', 'kernel' or 'host'; args.knn_route overrides

    def __init__(self, args, data):
        self._common_init(args, data, 'UserKNN')
        for k, conv in (('knn_k', int), ('knn_measure', str), ('knn_shrink', float), ('knn_route', str)):
            setattr(self, k, conv(getattr(args, k, getattr(type(self), k))))
        if self.knn_k < 1 or self.knn_measure not in neighbours.MEASURES or not self.knn_shrink >= 0.0 or self.knn_route not in itemknn.ROUTES:
            raise ValueError("UserKNN: knn_k >= 1, knn_measure in ('count', 'cosine', 'jaccard'), knn_shrink >= 0 and knn_route in ('auto', 'kernel', 'host')")
        self.device = 'cuda' if torch.cuda.is_available() else 'cpu'
        self.nbr_idx = self.nbr_cnt = self.nbr_w = self.user_deg = None
        self._X = self._dev_lists = None

    # ---- the model: the user-side lists of the training matrix
    def fit(self):
        """The user-side neighbour lists of the current training matrix: (nbr_idx, nbr_cnt int32 [U, knn_k], user_deg int64 [U]) and nbr_w."""
        X = self._matrix()
        U, I = X.shape
        idx, cnt, deg = neighbours.cooccur_topk(X.indptr.astype(np.int64), X.indices.astype(np.int32), U, I, self.knn_k, self.knn_measure,
                                                device=self.device, route=self.knn_route)
        self.nbr_idx, self.nbr_cnt, self.user_deg = idx.cpu().numpy(), cnt.cpu().numpy(), deg.cpu().numpy()
        self.nbr_w = itemknn.knn_weights(self.nbr_idx, self.nbr_cnt, self.user_deg, self.knn_measure, self.knn_shrink)
        self._X = X
        self._dev_lists = None

    def _score_topk(self, rows, N, mask, targets=None):
        """uknn_score_topk on the fitted lists, as numpy arrays."""
        self._fitted()
        X = self._X
        if self._dev_lists is None:                               # the lists travel to the device once
            dev = self.device if self.knn_route != 'host' else 'cpu'
            self._dev_lists = tuple(torch.from_numpy(a).to(dev) for a in (X.indptr.astype(np.int64), X.indices.astype(np.int32), self.nbr_idx, self.nbr_w))
        rp, ci, ni, nw = self._dev_lists
        idx, score, rank = userknn.uknn_score_topk(rp, ci, X.shape[0], X.shape[1], ni, nw, N, rows=None if rows is None else np.asarray(rows, np.int64),
                                                   mask_profile=mask, targets=targets, device=self.device, route=self.knn_route)
        return idx.cpu().numpy(), score.cpu().numpy(), None if rank is None else rank.cpu().numpy()

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5, requires_grad=False):
        if requires_grad:
            raise NotImplementedError('requires_grad is not implemented for UserKNN: its lists are counted, no gradient step is taken')
        if requires_embgrad:
            raise NotImplementedError('requires_embgrad is not implemented for UserKNN: the model has no embedding tables')
        if requires_adjgrad:
            raise NotImplementedError('requires_adjgrad is not implemented for UserKNN: the model has no adjacency')
        self.bestPerformance = []
        self.fit()
        print('training: neighbour lists of', self.nbr_idx.shape[0], 'users, k =', self.knn_k, 'measure:', self.knn_measure)
        self.evaluate(0)

    # ---- evaluation: KNNRecommender's, on _score_topk above
    def predict(self, u):
        """The dense float score row of user u (a raw id) over the whole catalogue."""
        self._fitted()
        q = self.data.get_user_id(u)
        row = np.asarray((userknn.weight_matrix(self.nbr_idx, self.nbr_w, self._X.shape[0], [q]) @ self._X).todense(), dtype=np.int64).ravel()
        return itemknn.float_score(row, self.knn_measure)

    def neighbours_of(self, user):
        """[(raw user id, float similarity)] of the fitted list of `user` (a raw id), best first."""
        self._fitted()
        u = self.data.get_user_id(user)
        sim = itemknn.knn_similarity(self.nbr_idx, self.nbr_cnt, self.user_deg, self.knn_measure, self.knn_shrink)[u]
        return [(self.data.id2user[int(v)], float(s)) for v, s in zip(self.nbr_idx[u], sim) if v >= 0]

    def neighbour_share(self, users):
        """float64 [U], in data.user's internal order: for every user the share of its list's summed weight held by the named raw user ids (an id
        the data does not know is ignored), 0 for an empty list.  With the fake ids: how far each neighbourhood is infiltrated.  Host arithmetic on
        the fitted integers: two int64 sums and one division per user."""
        self._fitted()
        named = np.zeros(self.nbr_idx.shape[0], bool)
        ids = [self.data.user[u] for u in users if u in self.data.user]
        named[np.asarray(ids, np.int64)] = True
        used = self.nbr_idx >= 0
        w = np.where(used, self.nbr_w.astype(np.int64), 0)
        held = np.where(used & named[np.where(used, self.nbr_idx, 0)], w, 0).sum(1)
        total = w.sum(1)
        return np.where(total > 0, held / np.maximum(total, 1), 0.0).astype(np.float64)

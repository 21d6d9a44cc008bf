"""iALS: WRMF as published (Hu, Koren, Volinsky, ICDM'08) -- implicit-feedback matrix factorisation that weighs EVERY unobserved pair and is solved
by alternating least squares, the victim the bilevel injection attacks are formulated against (Li et al., NIPS'16; Fang et al.; Tang et al.).  The
reference ships no such model: its WRMF (mirrored in recommender/WRMF.py, untouched) is a sampled SGD approximation of the objective.

    L = sum_u sum_i c_ui (p_ui - x_u . y_i)^2 + als_reg (|X|^2 + |Y|^2),   p = 1 on the training entries, c = 1 + als_alpha w there, 1 elsewhere

with w = 1 (als_weighting = 'binary') or the stored rating ('rating').  One epoch is one sweep: item Gram -> every user row -> user Gram -> every item
row, each row the exact minimiser given the other table (arlib_amd/als.py).  No sampler, no optimizer, and after the tables'
initialisation nothing is drawn from `random` or torch's generator.

The model is GMF's Matrix_Factorization: user_emb and item_emb are the two tables, so predict, test(), save, AttackMetric, TargetRankMetric and every
attack that reads the tables work unchanged through _base.Recommender.  fold_in() gives the row a new profile receives from the current item table
without retraining: the same row solve, on rows that are not in the model."""
import numpy as np
import scipy.sparse as sp
import torch

from ..als import gram, als_solve_rows, als_objective
from ._base import Recommender
from .GMF import Matrix_Factorization


class iALS(Recommender):
    als_alpha = 10.0                  # confidence of a stored entry: c = 1 + als_alpha w; args.als_alpha overrides
    als_reg = 0.1                     # lambda of both tables; args.als_reg overrides
    als_weighting = 'binary'          # w = 1 ('binary') or the stored rating ('rating'); args.als_weighting overrides
    als_route = 'auto'                # als_solve_rows' route: 'auto', 'fused' or 'composed'; args.als_route overrides

    def __init__(self, args, data):
        self._common_init(args, data, 'iALS')
        for k, conv in (('als_alpha', float), ('als_reg', float), ('als_weighting', str), ('als_route', str)):
            setattr(self, k, conv(getattr(args, k, getattr(type(self), k))))
        if not self.als_alpha >= 0.0 or not self.als_reg > 0.0 or self.als_weighting not in ('binary', 'rating') or self.als_route not in ('auto', 'fused', 'composed'):
            raise ValueError("iALS: als_alpha >= 0, als_reg > 0, als_weighting in ('binary', 'rating') and als_route in ('auto', 'fused', 'composed')")
        self.model = Matrix_Factorization(self.data, self.args.emb_size)
        self._csr = self._build_csr()
        self.sweeps_done = 0

    def _build_csr(self):
        """{'user': (rowptr, col[, val]), 'item': the transposed CSR}: int32 host tensors, one entry per distinct training pair (ratings of a repeated
        pair add up), built once."""
        data = self.data
        U, I = data.user_num, data.item_num
        if self.als_weighting == 'rating':
            td = data.training_data
            u = np.fromiter((data.user[r[0]] for r in td), dtype=np.int64, count=len(td))
            i = np.fromiter((data.item[r[1]] for r in td), dtype=np.int64, count=len(td))
            w = np.fromiter((float(r[2]) for r in td), dtype=np.float64, count=len(td))
            m = sp.csr_matrix((w, (u, i)), shape=(U, I))
        else:
            m = sp.csr_matrix(data.interaction_mat, dtype=np.float64)
        m.sum_duplicates(); m.eliminate_zeros(); m.sort_indices()
        out = {}
        for side, mat in (('user', m), ('item', sp.csr_matrix(m.T))):
            mat.sort_indices()
            csr = (torch.from_numpy(mat.indptr.astype(np.int32)), torch.from_numpy(mat.indices.astype(np.int32)))
            if self.als_weighting == 'rating':
                csr = csr + (torch.from_numpy(mat.data.astype(np.float32)),)
            out[side] = csr
        return out

    def _tables(self):
        e = self.model.embedding_dict
        return e['user_emb'], e['item_emb']

    def _side(self, side):
        """(the table solved, the other table, the CSR of the solved table's rows on the tables' device)."""
        if side not in ('user', 'item'):
            raise ValueError("iALS: side is 'user' or 'item', not %r" % (side,))
        u, i = self._tables()
        dev = u.device
        if self._csr[side][0].device != dev:
            self._csr = {k: tuple(t.to(dev) for t in v) for k, v in self._csr.items()}
        return (u, i, self._csr['user']) if side == 'user' else (i, u, self._csr['item'])

    def half_sweep(self, side):
        """Every row of the `side` table ('user' | 'item') replaced by its exact minimiser given the other table."""
        X, Y, csr = self._side(side)
        with torch.no_grad():
            Yc = Y.detach().contiguous()
            X.data.copy_(als_solve_rows(Yc, gram(Yc), csr, self.als_alpha, self.als_reg, route=self.als_route, check_range=False))

    def objective(self):
        """L of the current tables (a float), by the Gram identity."""
        u, i, csr = self._side('user')
        with torch.no_grad():
            return float(als_objective(u.detach().contiguous(), i.detach().contiguous(), csr, self.als_alpha, self.als_reg, check_range=False))

    def fold_in(self, rowptr, col, val=None):
        """User rows [n_profiles, d] for arbitrary profiles (CSR over the items: rowptr [n_profiles + 1], col int32[, val weights]) against the CURRENT
        item table, without retraining."""
        _, items = self._tables()
        dev = items.device
        csr = (rowptr.to(dev), col.to(dev)) + (() if val is None else (val.to(dev).float(),))
        with torch.no_grad():
            Yc = items.detach().contiguous()
            return als_solve_rows(Yc, gram(Yc), csr, self.als_alpha, self.als_reg, route=self.als_route, check_range=True)

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5, requires_grad=False):
        if requires_grad:
            raise NotImplementedError('requires_grad is not implemented for iALS: its tables are closed-form row solves, no gradient step is taken')
        if requires_embgrad:
            raise NotImplementedError('requires_embgrad is not implemented for iALS: a sweep computes no gradient of the tables to accumulate')
        if requires_adjgrad:
            raise NotImplementedError('requires_adjgrad is not implemented for iALS: the model has no adjacency')
        self.bestPerformance = []
        model = self.model.cuda() if torch.cuda.is_available() else self.model
        for epoch in range(Epoch if Epoch else self.args.maxEpoch):
            self.half_sweep('user')
            self.half_sweep('item')
            self.sweeps_done += 1
            print('training:', epoch + 1, 'objective:', self.objective())
            model.eval()
            self.user_emb, self.item_emb = self._detached_forward()
            if epoch % evalNum == 0:
                self.evaluate(epoch)
        self.user_emb, self.item_emb = self.best_user_emb, self.best_item_emb

    def _test_topk(self):
        if self.user_emb.is_cuda:
            return super()._test_topk()
        # tables on the CPU (a machine without a GPU trains through the composed route): Recommender._test_topk's own torch branch
        users = list(self.data.test_set)
        if not users:
            return users, np.zeros((0, 0), np.int64), np.zeros((0, 0), np.float32)
        uid = torch.tensor([self.data.user[u] for u in users], dtype=torch.long)
        sc = self.user_emb[uid] @ self.item_emb.T
        for r, u in enumerate(users):
            sc[r, [self.data.item[it] for it in self.data.training_set_u[u]]] = -10e8
        val, idx = torch.topk(sc, min(self.max_N, sc.shape[1]))
        return users, idx.numpy(), val.numpy()

"""LegUP (reference attack/Gray/LegUP.py): AUSH's discriminator phase, and a generator phase that retrains an own LightGCN on sampled graphs and
reads the ranking loss L_RS off it -- a softmax over the USERS of every item column of the U x I score matrix, which the reference materialises
(and a U x T x I tensor on top) and ops.colsoftmax_target streams (csrc/arl_colsoftmax.hip).

Interface and streams as in the reference: `LegUP(arg, data)`, `posionDataAttack(epoch1=25, epoch2=25)`, attributes G, D, selectItem, fakeUser,
fakeRat, lightgcn, Tepoch = 10, BiLevelOptimizationEpoch = 50, batchSize = 128.  The template, the D step and the final generation are AUSH's
(AUSH._template, _gan.d_step, AUSH._fake_profiles).  Every numpy and `random` draw happens on the host with the reference's calls in the
reference's order.  One G step (LegUP.py:99-175) is Tepoch times
    one more fake user who rated the targets (DLAttack.fakeUserInject, always named after row userNum: LegUP.py:137) -> the LightGCN re-initialised
    with its propagated tables carried over -> num_samples = np.random.randint(int(U * 0.1), int(I * 0.1)) edges of the grown interaction matrix
    drawn with np.random.choice(replace=False) in nonzero() order -> _init_uiAdj(sampled + sampled.T) -> train(Epoch=0) = a full maxEpoch
    training -> L_RS from the first userNum rows of Pu and all of Pi,
then `optimize_G.step()` on the last L_RS.

Kept quirks: L_RS does not depend on G, so G's parameters have no gradient and the step moves nothing -- G stays at its
initial values and loss2 is only logged (neither the backward nor the no-op step is spent here); the target columns of the score matrix are
indexed by the targets' POSITIONS in selectItem, not their item ids; np.random.randint raises ValueError when int(U * 0.1) >= int(I * 0.1);
lightgcn.data (the caller's data object) grows by one user per inner iteration.
"""
import hashlib
from types import SimpleNamespace

import numpy as np
import scipy.sparse as sp
import torch

from ..Black._shilling import remaining_ids
from ..White.DLAttack import DLAttack
from ...recommender.LightGCN import LightGCN
from ...util.sampler import sample_range
from ...util.optim import Adam
from ... import ops
from . import _gan
from .AUSH import AUSH, Generator, Discriminator, DEVICE


def default_recommender_args(**kw):
    """The reference's conf/recommend_parser.py defaults (what its LegUP builds its LightGCN from)."""
    a = dict(dataset='ml-1M', data_path='data/clean/', training_data='/train.txt', val_data='/val.txt', test_data='/test.txt', model_name='LightGCN',
             maxEpoch=30, batch_size=2048, emb_size=64, n_layers=2, reg=1e-4, lRate=0.005, dropout=True, dropout_rate=0.3, cuda=True, gpu_id='0',
             seed=2018, topK='50', load=True, save=True, save_dir='./modelsaved/')
    a.update(kw)
    return SimpleNamespace(**a)


def sample_edges(ui, n_real_users, n_items):
    """LegUP.py:139-149 on the host: num_samples = np.random.randint(int(U * 0.1), int(I * 0.1)) stored entries of the U' x I interaction matrix `ui`
    in nonzero() order (row-major, ascending columns), drawn with np.random.choice(nnz, num_samples, replace=False).  Returns (rows, cols) of the
    drawn entries.  randint raises ValueError when int(U * 0.1) >= int(I * 0.1), as in the reference."""
    m = sp.csr_matrix(ui)
    m.sort_indices()
    r, c = m.nonzero()
    num_samples = np.random.randint(int(n_real_users * 0.1), int(n_items * 0.1))
    sel = np.random.choice(len(r), num_samples, replace=False)
    return r[sel], c[sel]


def edge_digest(rows, cols):
    """SHA-256 of a sampled edge SET: the (row, col) pairs as int32, sorted by row then column."""
    o = np.lexsort((cols, rows))
    return hashlib.sha256(np.ascontiguousarray(rows[o], np.int32).tobytes() + np.ascontiguousarray(cols[o], np.int32).tobytes()).hexdigest()


def sampled_adjacency(rows, cols, n_users, n_items):
    """selected_ui_adj + selected_ui_adj.T (LegUP.py:150-156): the (U' + I)^2 symmetric 0/1 adjacency of the drawn edges."""
    N = n_users + n_items
    a = sp.csr_matrix((np.ones(len(rows), np.float32), (rows, cols + n_users)), shape=(N, N), dtype=np.float32)
    return a + a.T


class LegUP(AUSH):
    fakeUserInject = DLAttack.fakeUserInject       # one more user who rated the targets; tables carried over (the same code in both references)

    def __init__(self, arg, data, rec_args=None):
        super().__init__(arg, data)
        self.args = default_recommender_args() if rec_args is None else rec_args
        self.lightgcn = LightGCN(self.args, data)
        self.lightgcn.model = self.lightgcn.model.cuda()
        self.Tepoch = 10
        self.batchSize = 128
        self.sample_log = []               # (num_samples, edge_digest) of every sampled edge set, in order

    def ranking_loss(self):
        """L_RS of the own LightGCN as it stands (LegUP.py:160-171): the first userNum rows of Pu, all of Pi, target columns = the targets' positions
        in selectItem (the reference's indexing)."""
        with torch.no_grad():
            Pu, Pi = self.lightgcn.model()
            cols = [self.selectItem.index(t) for t in self.targetItem]
            return ops.colsoftmax_target(Pu[:self.userNum].contiguous(), Pi.contiguous(), cols)[0]

    def _g_step(self):
        rec = self.lightgcn
        loss = None
        for _ in range(self.Tepoch):
            self.fakeUserInject(rec, self.userNum)
            rows, cols = sample_edges(rec.data.matrix(), self.userNum, self.itemNum)
            self.sample_log.append((len(rows), edge_digest(rows, cols)))
            rec.model._init_uiAdj(sampled_adjacency(rows, cols, rec.data.user_num, self.itemNum))
            rec.train(requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5)
            loss = self.ranking_loss()
        return loss

    def posionDataAttack(self, epoch1=25, epoch2=25):
        if self.G is None:
            pool = remaining_ids(self.itemNum, self.targetItem)
            self.selectItem = pool[sample_range(len(pool), self.itemNum // 5)].tolist() + self.targetItem
            S, T = len(self.selectItem), len(self.targetItem)
            G = Generator(S)
            D = Discriminator(S)
            G, D = G.to(DEVICE), D.to(DEVICE)
            optimize_D = Adam(D.parameters(), lr=0.005)
            fused = self.fused()
            for i in range(self.BiLevelOptimizationEpoch):
                G.eval()
                D.train()
                for k1 in range(epoch1):
                    self.loss_log.append(_gan.d_step(G, D, optimize_D, self._template(), T, fused))
                D.eval()
                G.train()
                for k2 in range(epoch2):
                    self.loss_log.append(self._g_step())           # no gradient reaches G: nothing to step
            self.G = G
            self.D = D
        return self._fake_profiles()

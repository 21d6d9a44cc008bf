"""WRMF -- mirror of the reference's recommender/WRMF.py (class WRMF :15-149, Matrix_Factorization :151-175): GMF's matrix factorisation
trained with wrmf_loss + l2_reg_loss (util/loss.py:11-15, 25-29) instead of BPR, on the fused WRMF kernel (util.loss.wrmf_l2_loss).
Matrix_Factorization is GMF's: forward() returns the Parameters themselves (the reference's aliasing of user_emb / best_user_emb kept); as in
the reference's own copy of the class, it has no graph to rebuild."""
from ..util.loss import wrmf_l2_loss
from ._base import Recommender
from . import GMF


class Matrix_Factorization(GMF.Matrix_Factorization):
    def _init_uiAdj(self, *args):
        raise Exception("This model hava no graph")          # recommender/WRMF.py:168-169


class WRMF(Recommender):
    def __init__(self, args, data):
        self._common_init(args, data, 'WRMF')
        self.model = Matrix_Factorization(self.data, args.emb_size)

    def _batch_loss(self, user_emb, pos_item_emb, neg_item_emb, reg):
        return wrmf_l2_loss(user_emb, pos_item_emb, neg_item_emb, reg)

    def _fusable(self, optimizer):
        return None                          # the fused engine step is BPR-only: WRMF always runs the caller's optimizer through autograd

    def train(self, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5):
        return self._train_loop(Epoch, optimizer, evalNum, requires_embgrad=requires_embgrad, gradIterationNum=gradIterationNum)

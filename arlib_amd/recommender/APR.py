"""APR / AMF: Adversarial Personalized Ranking (He et al., SIGIR'18) -- BPR + L2 plus BPR under the worst-case first-order perturbation of the rows the
scorer reads.  The reference ships attacks and no defended victim; this is the paper's model on the reference's own pieces (Matrix_Factorization or
LGCN_Encoder, next_batch_pairwise, bpr_loss, l2_reg_loss):

    loss = bpr_loss(u, p, n) + l2_reg_loss(reg, u, p) + adv_reg * bpr_loss(u + delta_u, p + delta_p, n + delta_n)
    delta_r = eps * Gamma_r / max(||Gamma_r||, 1e-6),  Gamma_r = d bpr_loss / d(row of node r), summed over the batch positions that name r

with delta a constant of the step.  Departures from the paper, all listed in DESIGN.md section 6: the normalisation is
row-wise (the authors' implementation; the paper bounds the whole perturbation), the L2 term reads the clean rows only and is un-squared (quirk Q8),
and with encoder = 'lightgcn' the perturbation lives on the PROPAGATED rows (the scorer's inputs), not on the embedding table.  Epochs before
adv_start_epoch run the plain BPR step: the authors' pretraining phase.  The term is one kernel call (ops.bpr_adv_fwd_bwd) in the fused step
(engine.step_apr) and in the autograd route (util.loss.adv_bpr_loss)."""
import torch

from .. import ops
from ..util.loss import adv_bpr_loss, bpr_loss
from ._base import Recommender
from .GMF import Matrix_Factorization
from .LightGCN import LGCN_Encoder


class APR(Recommender):
    print_every = 100
    eps = 0.5                         # size of each node's perturbation; args.apr_eps overrides
    adv_reg = 1.0                     # weight of the adversarial term; args.apr_reg overrides
    adv_start_epoch = 0               # first epoch (0-based, counted over the object's life) with the adversarial term; args.apr_start_epoch overrides
    encoder = 'mf'                    # 'mf' (APR as published) or 'lightgcn' (args.n_layers hops); args.apr_encoder overrides

    def __init__(self, args, data):
        self._common_init(args, data, 'APR')
        self.eps = float(getattr(args, 'apr_eps', type(self).eps))
        self.adv_reg = float(getattr(args, 'apr_reg', type(self).adv_reg))
        self.adv_start_epoch = int(getattr(args, 'apr_start_epoch', type(self).adv_start_epoch))
        self.encoder = getattr(args, 'apr_encoder', type(self).encoder)
        if self.encoder == 'mf':
            self.model = Matrix_Factorization(self.data, self.args.emb_size)
        elif self.encoder == 'lightgcn':
            self.model = LGCN_Encoder(self.data, self.args.emb_size, self.args.n_layers)
        else:
            raise ValueError("APR: apr_encoder must be 'mf' or 'lightgcn', got %r" % (self.encoder,))
        self._epochs_begun = 0
        self._batch_index = None
        self.last_adv_loss = torch.zeros(())

    def _adversarial(self):
        return self._epochs_begun > self.adv_start_epoch

    def _on_epoch_start(self, model):
        self._epochs_begun += 1

    def _fusable(self, optimizer):
        """The base rule, within the adversarial kernel's limits (past them the autograd route composes the term from torch ops)."""
        return super()._fusable(optimizer) if ops.bpr_adv_supported(self.args.batch_size, self.args.emb_size) else None

    def _fused_step(self, eng, u, p, n):
        if not self._adversarial():
            self.last_adv_loss = torch.zeros(())
            return eng.step(u, p, n)
        lo, self.last_adv_loss = eng.step_apr(u, p, n, eps=self.eps, adv_reg=self.adv_reg)
        return lo

    def _batch_loss(self, user_emb, pos_item_emb, neg_item_emb, reg):
        self._rec_rows = tuple(t.detach() for t in (user_emb, pos_item_emb, neg_item_emb))       # for the training line only
        loss = super()._batch_loss(user_emb, pos_item_emb, neg_item_emb, reg)
        if not self._adversarial():
            self.last_adv_loss = torch.zeros(())
            return loss
        if self._batch_index is None:
            raise RuntimeError('APR: the adversarial term needs the batch\'s node ids, which only train() supplies on the autograd route')
        ul, pl, nl = self._batch_index
        U = self.data.user_num
        adv = self.adv_reg * adv_bpr_loss(user_emb, pos_item_emb, neg_item_emb, self.eps, groups=torch.cat([ul, pl + U, nl + U]))
        self.last_adv_loss = adv.detach()          # detached: the recommender stays copyable and picklable after training
        return loss + adv

    def _print_step(self, epoch, n, lo=None, batch_loss=None):
        if lo is not None:
            rec = float(lo[0])
        else:
            with torch.no_grad():
                rec = bpr_loss(*self._rec_rows).item()
        print('training:', epoch + 1, 'batch', n, 'rec_loss:', rec, 'adv_loss', float(self.last_adv_loss))

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5):
        try:
            return self._train_loop(Epoch, optimizer, evalNum, requires_embgrad=requires_embgrad, requires_adjgrad=requires_adjgrad,
                                    gradIterationNum=gradIterationNum)
        finally:
            self._batch_index = self._rec_rows = None          # batch-sized device tensors of the last step: not part of the trained object

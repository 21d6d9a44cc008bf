"""DirectAU (Wang et al., KDD'22) on the LightGCN encoder: the one published model util/loss.py:17-23 (alignment_loss, uniformity_loss) were written
for.  The reference ships the two loss functions and no model file; this is DirectAU's public SELFRec form on the reference's own pieces
(LGCN_Encoder, next_batch_pairwise, l2_reg_loss):

    loss = alignment_loss(u, p) + gamma * (uniformity_loss(u) + uniformity_loss(p)) / 2 + l2_reg_loss(reg / batch_size, u, p)

on the batch's propagated user rows u and positive-item rows p, duplicates kept.  The sampler still draws the negatives (the `random` stream is
LightGCN's), the loss does not read them.  Both terms run the kernels of arlib_amd/pairloss.py."""
from ..util.loss import alignment_loss, uniformity_loss, l2_reg_loss
from ._base import Recommender
from .LightGCN import LGCN_Encoder


class DirectAU(Recommender):
    gamma = 2.0                       # weight of the uniformity term; args.directau_gamma overrides
    l2_scale = None                   # 1 / batch_size, set per instance

    def __init__(self, args, data):
        self._common_init(args, data, 'DirectAU')
        self.gamma = float(getattr(args, 'directau_gamma', type(self).gamma))
        self.l2_scale = 1.0 / self.args.batch_size
        self.model = LGCN_Encoder(self.data, self.args.emb_size, self.args.n_layers)

    def _batch_loss(self, user_emb, pos_item_emb, neg_item_emb, reg):
        return (alignment_loss(user_emb, pos_item_emb) + self.gamma * (uniformity_loss(user_emb) + uniformity_loss(pos_item_emb)) / 2
                + l2_reg_loss(reg, user_emb, pos_item_emb))

    def _fusable(self, optimizer):
        return None                          # the fused engine step is BPR-only: DirectAU always runs the caller's optimizer through autograd

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5):
        return self._train_loop(Epoch, optimizer, evalNum, requires_embgrad=requires_embgrad, requires_adjgrad=requires_adjgrad,
                                gradIterationNum=gradIterationNum)

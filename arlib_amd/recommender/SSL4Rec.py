"""SSL4Rec: the LightGCN mean over layers 0..2, BPR + L2, plus InfoNCE between two dropout views of the batch's propagated user rows and of its
positive-item rows (drop 0.2, tau 0.2, cl_rate 1) -- mirror of the reference's recommender/SSL4Rec.py (class SSL4Rec :18-166, DNN_Encoder
:169-247) on the MI355X kernels.

The contrastive term is one kernel call (ops.ssl_dropout_nce: both views, both sides, forward and backward).  The fused step
(engine.step_ssl4rec) adds its gradient into the compact batch gradient of the sparse-batch step; the autograd route wraps the same kernel
in _DropoutNce.  Dropout masks are drawn inside the kernel from a seed taken once from torch's generator and a running stream number, one
per step (the reference's nn.Dropout draws cannot be reproduced).  Widths outside ops.SSL_NCE_WIDTHS take nn.Dropout + InfoNCE.
"""
import torch
import torch.nn as nn

from .. import ops
from ._base import DEVICE, GraphEncoder, Recommender, TorchGraphInterface
from ..util.loss import InfoNCE, bpr_loss
from ..util.optim import Adam as FusedAdam


class _DropoutNce(torch.autograd.Function):
    """(Xu, Xp) -> [InfoNCE of the user views, InfoNCE of the positive views]; the kernel computes both gradients in the forward call."""

    @staticmethod
    def forward(ctx, Xu, Xp, drop, tau, seed, stream_id, masks):
        loss, G = ops.ssl_dropout_nce(Xu.contiguous(), Xp.contiguous(), drop, tau, seed=seed, stream_id=stream_id, masks=masks)
        ctx.save_for_backward(*G)
        return loss

    @staticmethod
    def backward(ctx, g):
        Gu, Gp = ctx.saved_tensors
        return Gu * g[0], Gp * g[1], None, None, None, None, None


class DNN_Encoder(GraphEncoder):
    n_prop_layers = 2

    def __init__(self, data, emb_size, drop_rate, temperature, n_layers):
        nn.Module.__init__(self)
        self.data = data
        self.latent_size = self.emb_size = emb_size
        self.tau = temperature
        self.drop_rate = drop_rate
        # the reference's creation order (SSL4Rec.py:174-191): both towers and the dropout, then _init_model() twice (the first draw is discarded).
        # The towers are parameters that forward() never uses (:227-228 are commented out).
        self.user_tower = nn.Sequential(nn.Linear(self.emb_size, 1024), nn.ReLU(True), nn.Linear(1024, 128), nn.Tanh())
        self.item_tower = nn.Sequential(nn.Linear(self.emb_size, 1024), nn.ReLU(True), nn.Linear(1024, 128), nn.Tanh())
        self.dropout = nn.Dropout(drop_rate)
        self.embedding_dict = self._init_model()
        self.layers = self.n_prop_layers = n_layers
        self.norm_adj = data.norm_adj
        self.embedding_dict = self._init_model()
        self.sparse_norm_adj = TorchGraphInterface.convert_sparse_mat_to_tensor(self.norm_adj)
        self._eng = None
        self.mask_seed = None          # taken from torch's generator at the first contrastive term
        self.mask_stream = 0           # one stream per step
        self.view_masks = None         # optional callable(stream, B, d) -> bool [2 sides][2 views][B][d] (parity tests)

    def cuda(self, device=None):
        self._pack()
        for t in self.tower_parameters():
            if not t.is_cuda:
                t.data = t.data.to(DEVICE)
        return self

    def tower_parameters(self):
        return list(self.user_tower.parameters()) + list(self.item_tower.parameters())

    def next_masks(self, B):
        """(seed, stream, masks) of the next contrastive term over B positions."""
        if self.mask_seed is None:
            self.mask_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        stream = self.mask_stream
        self.mask_stream += 1
        return self.mask_seed, stream, (self.view_masks(stream, B, self.latent_size) if self.view_masks is not None else None)

    def cal_cl_loss(self, user_rows, pos_rows):
        """recommender/SSL4Rec.py:232-247 on the step's propagated rows user_rows = rec_user_emb[uidx], pos_rows = rec_item_emb[iidx]:
        InfoNCE(item views) + InfoNCE(user views)."""
        seed, stream, masks = self.next_masks(user_rows.shape[0])
        if self.latent_size in ops.SSL_NCE_WIDTHS:
            loss = _DropoutNce.apply(user_rows, pos_rows, self.drop_rate, self.tau, seed, stream, masks)
            return loss[1] + loss[0]
        if masks is not None:
            s = 1.0 / (1.0 - self.drop_rate)
            u1, u2, i1, i2 = (x * m * s for x, m in ((user_rows, masks[0, 0]), (user_rows, masks[0, 1]), (pos_rows, masks[1, 0]), (pos_rows, masks[1, 1])))
        else:
            u1, u2, i1, i2 = self.dropout(user_rows), self.dropout(user_rows), self.dropout(pos_rows), self.dropout(pos_rows)
        return InfoNCE(i1, i2, self.tau) + InfoNCE(u1, u2, self.tau)


class SSL4Rec(Recommender):
    print_every = 100
    has_extra_loss = True
    fused_extra_loss = True
    extra_loss_takes_outputs = True
    adjgrad_through_views = True

    def __init__(self, args, data):
        self._common_init(args, data, 'SSL4Rec')
        # Hyperparameter (SSL4Rec.py:29-34)
        self.n_layers = 2
        self.cl_rate = 1
        self.tau = 0.2
        self.drop_rate = 0.2
        self.model = DNN_Encoder(self.data, self.args.emb_size, self.drop_rate, self.tau, self.n_layers)

    def _fusable(self, optimizer):
        """The fused step stands in for a stock Adam over the two tables, alone or with the towers (the default Adam(model.parameters())): the
        towers never receive a gradient, so Adam never moves them."""
        if type(optimizer) not in (torch.optim.Adam, FusedAdam) or len(optimizer.param_groups) != 1 or self.model.latent_size not in ops.SSL_NCE_WIDTHS:
            return None
        g = optimizer.param_groups[0]
        towers = {id(t) for t in self.model.tower_parameters()}
        ps = [p for p in g['params'] if id(p) not in towers]
        n_towers = len(g['params']) - len(ps)
        mine = self._params()
        if n_towers not in (0, len(towers)) or len(ps) != 2 or {id(ps[0]), id(ps[1])} != {id(mine[0]), id(mine[1])}:
            return None
        if g.get('weight_decay', 0) != 0 or g.get('maximize', False) or g.get('amsgrad', False) or g.get('capturable', False):
            return None
        return 'adam'

    def _fused_step(self, eng, u, p, n):
        seed, stream, masks = self.model.next_masks(u.numel())
        lo, self.last_cl_loss = eng.step_ssl4rec(u, p, n, cl_rate=self.cl_rate, tau=self.tau, drop=self.drop_rate, masks=masks, seed=seed, stream_id=stream)
        return lo

    def _batch_loss(self, user_emb, pos_item_emb, neg_item_emb, reg):
        self._rec_rows = tuple(t.detach() for t in (user_emb, pos_item_emb, neg_item_emb))       # for the training line only
        return super()._batch_loss(user_emb, pos_item_emb, neg_item_emb, reg)

    def _extra_loss(self, model, user_idx, pos_idx, rec_user_emb, rec_item_emb):
        cl = self.cl_rate * model.cal_cl_loss(rec_user_emb[user_idx], rec_item_emb[pos_idx])
        self.last_cl_loss = cl.detach()            # detached: the recommender stays copyable and picklable after training
        return cl

    def _print_step(self, epoch, n, lo=None, batch_loss=None):
        """SSL4Rec.py:72-73: the BPR term and the contrastive term."""
        if lo is not None:
            rec = float(lo[0])
        else:
            with torch.no_grad():
                rec = bpr_loss(*self._rec_rows).item()
        print('training:', epoch + 1, 'batch', n, 'rec_loss:', rec, 'cl_loss', float(self.last_cl_loss))

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5):
        return self._train_loop(Epoch, optimizer, evalNum, requires_embgrad=requires_embgrad, requires_adjgrad=requires_adjgrad,
                                gradIterationNum=gradIterationNum)

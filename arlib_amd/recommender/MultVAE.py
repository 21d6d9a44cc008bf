"""Mult-VAE and Mult-DAE (Liang et al., WWW'18): the autoencoder recommenders with a multinomial likelihood -- the INDUCTIVE victim: a user's
representation is computed from its profile, so an injected profile shifts the shared weights and has no row of its own to train.  The reference
ships no such model; this is the paper's model on the reference's own pieces (the interaction matrix, l2_reg_loss, Recommender's evaluation):

    x~_u = x_u / |x_u|_2 (x_u the binary training profile),   [mu | logvar] = dropout(x~_u) W_enc + b_enc,   z = mu + eps exp(logvar / 2),
    logits = z W_dec^T,   loss = mean_b nll_b + beta_t mean_b KL_b + vae_reg l2_reg_loss(W_enc, W_dec),
    KL_b = 1/2 sum_j (mu^2 + exp(logvar) - logvar - 1),   beta_t = vae_beta min(1, t / vae_anneal_steps) after t completed steps

with nll the multinomial likelihood over EVERY item (arlib_amd/multinomial.py).  vae_variational = False gives Mult-DAE: z = mu,
no KL, W_enc [I, d].  Dropout is torch's: kept entries are scaled by 1 / (1 - vae_dropout).

Two departures from the paper, both listed in DESIGN.md section 6: the decoder has NO OUTPUT BIAS and there are NO HIDDEN LAYERS (encoder and
decoder are one linear map each).  With them user_emb = mu of every user (no dropout, no sampling) and item_emb = W_dec are the model: user_emb @
item_emb.T IS its ranking, so predict, test(), save, AttackMetric, TargetRankMetric and every attack that only reads the two tables work unchanged
through _base.Recommender.  The op takes "last activation" and "last weight", so hidden layers would be plain torch around it.

Training batches are batches of USERS (random.shuffle of the user ids per epoch, sliced by vae_batch_users; no BPR sampler).  One step is a pure
function of (rows, keep, eps): keep [nnz of the batch's profiles] the per-edge dropout keep flags in CSR order, eps [B, d]."""
import random

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from .. import ops
from ..allpairs import transpose_positives
from ..multinomial import multinomial_nll
from ..util.loss import l2_reg_loss
from ._base import Recommender


def _sparse_rows(rowptr, col, val, W):
    """out [n_rows, N] = CSR (rowptr int64, col int32, val) x W [*, N], entries in CSR order: ops.gan_spmm on the GPU, index_add_ on the CPU (whose
    order is fixed too)."""
    if W.is_cuda:
        return ops.gan_spmm(rowptr, col, val, W, check_range=False)
    n = rowptr.numel() - 1
    r = torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1], output_size=col.numel())
    return torch.zeros(n, W.shape[1], dtype=W.dtype).index_add_(0, r, val.to(W.dtype)[:, None] * W[col.long()])


class _BatchEncode(torch.autograd.Function):
    """h [B, N] = the batch CSR's values x W_enc [I, N].  The weight gradient runs the same product through the TRANSPOSED batch CSR (a sort by item:
    a fixed order, unlike index_add_ on the GPU)."""

    @staticmethod
    def forward(ctx, W, rowptr, col, val, trowptr, trow, tval):
        ctx.save_for_backward(trowptr, trow, tval)
        return _sparse_rows(rowptr, col, val, W.contiguous())

    @staticmethod
    def backward(ctx, dh):
        trowptr, trow, tval = ctx.saved_tensors
        return _sparse_rows(trowptr, trow, tval, dh.contiguous()), None, None, None, None, None, None


class MultVAE_Encoder(nn.Module):
    n_prop_layers = 1                 # for Recommender._detached_forward: the tables it returns are computed, not the live parameters

    def __init__(self, data, emb_size, variational=True):
        super().__init__()
        self.data, self.latent_size, self.variational = data, int(emb_size), bool(variational)
        I, d = data.item_num, self.latent_size
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({'W_enc': nn.Parameter(init(torch.empty(I, 2 * d if self.variational else d))),
                                                'b_enc': nn.Parameter(torch.zeros(2 * d if self.variational else d)),
                                                'W_dec': nn.Parameter(init(torch.empty(I, d)))})
        # x_u: one entry per distinct training interaction, whatever its rating
        m = sp.csr_matrix(data.interaction_mat)
        m.sum_duplicates(); m.eliminate_zeros(); m.sort_indices()
        self.rowptr = torch.from_numpy(m.indptr.astype(np.int64))
        self.col = torch.from_numpy(m.indices.astype(np.int32))
        deg = torch.from_numpy(np.diff(m.indptr).astype(np.float64))
        self.inv_norm = torch.where(deg > 0, deg.clamp(min=1).rsqrt(), torch.zeros_like(deg)).float()        # 1 / |x_u|_2, 0 for an empty profile
        self._table = None

    @property
    def device(self):
        return self.embedding_dict['W_dec'].device

    def cuda(self, device=None):
        super().cuda(device)
        return self._move()

    def _move(self):
        dev = self.device
        if self.rowptr.device != dev:
            self.rowptr, self.col, self.inv_norm = self.rowptr.to(dev), self.col.to(dev), self.inv_norm.to(dev)
            self._table = None
        return self

    def batch_csr(self, rows):
        """The profiles of the users `rows` [B] (int64, on the model's device): (rowptr int64 [B + 1], col int32 [nnz], scale [nnz] = 1 / |x_u|_2)."""
        self._move()
        lo, deg = self.rowptr[rows], self.rowptr[rows + 1] - self.rowptr[rows]
        rowptr = torch.zeros(rows.numel() + 1, dtype=torch.int64, device=rows.device)
        rowptr[1:] = torch.cumsum(deg, 0)
        nnz = int(rowptr[-1])
        owner = torch.repeat_interleave(torch.arange(rows.numel(), device=rows.device), deg, output_size=nnz)
        at = lo[owner] + (torch.arange(nnz, device=rows.device) - rowptr[:-1][owner])
        return rowptr, self.col[at].contiguous(), self.inv_norm[rows][owner].contiguous()

    def step_loss(self, rows, keep, eps, beta, reg=0.0, dropout=0.5, route='auto'):
        """(loss, mean nll, mean KL) of one step, differentiable in the three weights: a pure function of (rows, keep, eps)."""
        W_enc, b_enc, W_dec = (self.embedding_dict[k] for k in ('W_enc', 'b_enc', 'W_dec'))
        dev, B, d, I = self.device, rows.numel(), self.latent_size, W_dec.shape[0]
        rows = rows.to(dev).long()
        rowptr, col, scale = self.batch_csr(rows)
        if keep.numel() != col.numel() or (self.variational and tuple(eps.shape) != (B, d)):
            raise ValueError('MultVAE: keep has one flag per stored entry of the batch\'s profiles (%d) and eps is [B, d]' % col.numel())
        val = (scale * keep.to(dev).to(scale.dtype) / (1.0 - dropout)).to(W_enc.dtype)
        rowptr32 = rowptr.to(torch.int32)
        trowptr, trow, perm = transpose_positives(rowptr32, col, B, I)
        h = _BatchEncode.apply(W_enc, rowptr, col, val, trowptr.long(), trow, val[perm.long()].contiguous()) + b_enc
        mu = h[:, :d]
        if self.variational:
            logvar = h[:, d:]
            z = mu + eps.to(dev).to(h.dtype) * torch.exp(0.5 * logvar)
            kl = 0.5 * (mu * mu + torch.exp(logvar) - logvar - 1.0).sum(1).mean()
        else:
            z, kl = mu, torch.zeros((), dtype=h.dtype, device=dev)
        nll = multinomial_nll(z, W_dec, (rowptr32, col), route=route, check_range=False).mean()
        loss = nll + beta * kl
        if reg:
            loss = loss + l2_reg_loss(reg, W_enc, W_dec)
        return loss, nll.detach(), kl.detach()

    def encode_all(self):
        """mu of every user, no dropout and no sampling: diag(1 / |x_u|_2) X W_enc[:, :d] + b_enc[:d]."""
        self._move()
        d = self.latent_size
        W, b = self.embedding_dict['W_enc'].detach()[:, :d].contiguous(), self.embedding_dict['b_enc'].detach()[:d]
        if not W.is_cuda:
            return _sparse_rows(self.rowptr, self.col, self.inv_norm[torch.repeat_interleave(torch.arange(self.inv_norm.numel()), self.rowptr[1:] - self.rowptr[:-1])], W) + b
        if self._table is None or self._table.device != W.device:
            self._table = ops.CSRGraph(self.rowptr.cpu().numpy(), self.col, torch.ones(self.col.numel(), device=W.device), W.device, n_cols=W.shape[0])
        return ops.spmm(self._table, W, row_scale=self.inv_norm) + b

    def forward(self):
        return self.encode_all(), self.embedding_dict['W_dec']

    def __getstate__(self):
        st = dict(self.__dict__)
        st['_table'] = None
        return st


class MultVAE(Recommender):
    print_every = 100
    vae_beta = 0.2                    # cap of the KL weight; args.vae_beta overrides
    vae_anneal_steps = 20000          # steps over which the KL weight rises linearly from 0 to its cap; args.vae_anneal_steps overrides
    vae_dropout = 0.5                 # dropout on the normalised input profile; args.vae_dropout overrides
    vae_batch_users = 500             # users per step; args.vae_batch_users overrides
    vae_reg = 0.0                     # weight of l2_reg_loss(W_enc, W_dec); args.vae_reg overrides
    vae_variational = True            # False: Mult-DAE; args.vae_variational overrides
    vae_route = 'auto'                # multinomial_nll's route: 'auto', 'fused' or 'composed'; args.vae_route overrides

    def __init__(self, args, data):
        self._common_init(args, data, 'MultVAE')
        for k, conv in (('vae_beta', float), ('vae_anneal_steps', int), ('vae_dropout', float), ('vae_batch_users', int), ('vae_reg', float),
                        ('vae_variational', bool), ('vae_route', str)):
            setattr(self, k, conv(getattr(args, k, getattr(type(self), k))))
        if not 0.0 <= self.vae_dropout < 1.0 or self.vae_batch_users < 1 or self.vae_route not in ('auto', 'fused', 'composed'):
            raise ValueError("MultVAE: 0 <= vae_dropout < 1, vae_batch_users >= 1 and vae_route in ('auto', 'fused', 'composed')")
        self.model = MultVAE_Encoder(self.data, self.args.emb_size, self.vae_variational)
        self.steps_done = 0
        self.last_losses = None

    def _params(self):
        return [self.model.embedding_dict[k] for k in ('W_enc', 'b_enc', 'W_dec')]

    def beta(self):
        """The KL weight of the next step."""
        if not self.vae_variational:
            return 0.0
        return self.vae_beta * (min(1.0, self.steps_done / self.vae_anneal_steps) if self.vae_anneal_steps > 0 else 1.0)

    def draw(self, rows):
        """(keep, eps) of a batch from torch's generator (the CPU one, after seedSet): what train() hands to step()."""
        nnz = int((self.model.rowptr[rows + 1] - self.model.rowptr[rows]).sum())
        keep = torch.rand(nnz) >= self.vae_dropout
        eps = torch.randn(len(rows), self.model.latent_size) if self.vae_variational else None
        return keep, eps

    def step(self, rows, keep, eps, optimizer):
        """One training step on the users `rows` with the keep flags and eps given: a pure function of them and of the weights."""
        model = self.model
        rows = torch.as_tensor(rows, dtype=torch.int64, device=model.device)
        loss, nll, kl = model.step_loss(rows, keep, eps, self.beta(), self.vae_reg, self.vae_dropout, self.vae_route)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        self.steps_done += 1
        self.last_losses = (loss.detach(), nll, kl)
        return self.last_losses

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5, requires_grad=False):
        if requires_grad:
            raise NotImplementedError('requires_grad is not implemented for MultVAE: its tables are computed from the profiles, not trained rows')
        if requires_embgrad:
            raise NotImplementedError('requires_embgrad is not implemented for MultVAE: user_emb is computed from the profiles and has no gradient of its own')
        if requires_adjgrad:
            raise NotImplementedError('requires_adjgrad is not implemented for MultVAE: the model has no adjacency')
        self.bestPerformance = []
        model = self.model.cuda() if torch.cuda.is_available() else self.model
        if optimizer is None:
            optimizer = torch.optim.Adam(self._params(), lr=self.args.lRate)
        self.optimizer = optimizer
        U = self.data.user_num
        for epoch in range(Epoch if Epoch else self.args.maxEpoch):
            users = list(range(U))
            random.shuffle(users)
            model.train()
            for n, b in enumerate(range(0, U, self.vae_batch_users)):
                rows = torch.tensor(users[b:b + self.vae_batch_users], dtype=torch.int64)
                keep, eps = self.draw(rows.to(model.rowptr.device))
                loss, nll, kl = self.step(rows, keep, eps, optimizer)
                if n % self.print_every == 0:
                    print('training:', epoch + 1, 'batch', n, 'nll:', float(nll), 'kl:', float(kl), 'beta:', self.beta())
            model.eval()
            self.user_emb, self.item_emb = self._detached_forward()
            if epoch % evalNum == 0:
                self.evaluate(epoch)
        self.user_emb, self.item_emb = self.best_user_emb, self.best_item_emb

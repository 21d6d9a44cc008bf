"""GSPAttack -- the attack the reference's attack/Black/GSPAttack.py describes, on the MI355X kernels: a generative surrogate (an NGCF proxy over the
poisoned bipartite graph), a relaxed k-hot fake profile per fake user drawn by Gumbel top-k from an MLP over pairs of proxy embeddings, and the loss
alpha * L_per + beta * L_exPR.  Same constructor attributes and protocol (`posionDataAttack()` takes no recommender and returns the scipy (U+F) x I
matrix, also stored in `self.interact`).

The reference's file cannot run as written; these six repairs give the attack it describes:
  1. Item node ids (GSPAttack.py:149-159): NGCFProxy puts item columns at node ids 0..I-1, where they alias user nodes; nodes past max(U+F, I) get
     d^-1/2 = inf, the loss is NaN and bestAdj is never bound.  Here nodes are users 0..R-1, then items R..R+I-1 (R = U + F).
  2. Softmax over one column (GSPAttack.py:201-202, 224-231): Gumbel_Softmax is called on an [I, 1] column, so its softmax runs over a dimension of
     size 1 and every fake edge ends up with the value k.  Here the softmax of every round runs over the items (gumbel_topk_relaxed).
  3. Mask by multiplication (GSPAttack.py:228-229): `x * mask` with mask = -10e9 turns negative logits into huge positive ones.  Here a picked item
     gets the additive mask -inf for all later rounds.
  4. No gradient to the MLP (GSPAttack.py:204): writes through adj_mat._values() carry no gradient, so the MLP never learns.  Here one hop of the
     poisoned graph is an autograd node with gradients to its operand and to the fake block S (PGA's formula, attack/White/PGA.py header).
  5. Stale best snapshot (GSPAttack.py:89-91): bestAdj = recommender.adj_mat keeps a reference to a tensor later epochs overwrite.  Here the best
     S is a copy; no finite loss in any epoch raises RuntimeError instead of the reference's unbound variable.
  6. Undefined attribute (GSPAttack.py:40): self.item_num is read before it exists.  Here a fractional maliciousFeedbackSize uses data.item_num.

Mechanics: the real users' part of L_per (a binary cross-entropy over all U x I scores; GSPAttack.py:63-75 materialises them on the CPU) streams
through ops.bce_allpairs (csrc/arl_allpairs.hip) with the reference's batched-mean weights (ops.batch_mean_row_weights); the fake users' F x I panel,
L_exPR and the MLP are plain torch.  The hop reuses PGA's FactoredFakeGraph and ops.sddmm_rows_dense, a layer is ops.ngcf_dense_fwd / _bwd.  The dense
F x I block is the size limit, as in PGA.

The profile generator has two routes (attribute profile_route, set on the instance before posionDataAttack): 'composed', the default, is the MLP
one fake user at a time and gumbel_topk_relaxed, both plain torch; 'fused' forms the first layer's two halves with two GEMMs and runs
ops.pair_mlp_logits_auto and ops.gumbel_topk_auto (csrc/arl_profilegen.hip; the composed routes past the kernels' limits).  noise_source 'torch'
(the default) draws self._noise((k, F, I)) on both routes; 'hash' draws one seed per attack from Python's random and takes the noise from a counter
hash of (seed, epoch, round, fake user, item): the fused route regenerates it inside the kernels, so no [k, F, I] tensor exists (the composed
route writes the same draw out with ops.gumbel_noise).
"""
import math
import random

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from ... import ops
from ...util.optim import Adam
from .._common import AttackBase, DEVICE
from ..White.PGA import FactoredFakeGraph

EPS = 10e-8            # the reference's literal (GSPAttack.py:73), = 1e-7
S_INIT = 1e-4          # the fake edges' initial weight (GSPAttack.py:158)


def gumbel_topk_relaxed(x, k, tau=1.0, noise=None, generator=None):
    """Relaxed k-hot rows by k rounds of Gumbel softmax without replacement.  x [F, I] logits.  Round r: y_r = softmax((x + m + g_r) / tau, dim=1)
    over the items, j = argmax y_r, m[f, j] = -inf for all later rounds; S = sum_r y_r.  g_r = -log(Exponential(1)) as F.gumbel_softmax draws it;
    noise [k, F, I] overrides the draw.  Returns (S [F, I], picks [F, k] int64).  Every row of S sums to k; single entries may exceed 1.
    Pure torch, differentiable in x, on CPU and GPU."""
    if x.dim() != 2 or not 1 <= k <= x.shape[1]:
        raise ValueError('gumbel_topk_relaxed: x [F, I] and 1 <= k <= I')
    if noise is not None and tuple(noise.shape) != (k,) + tuple(x.shape):
        raise ValueError('gumbel_topk_relaxed: noise [k, F, I]')
    m = torch.zeros_like(x)
    S = torch.zeros_like(x)
    picks = []
    for r in range(k):
        g = noise[r] if noise is not None else -torch.empty_like(x).exponential_(generator=generator).log()
        y = torch.softmax((x + m + g) / tau, dim=1)
        j = torch.argmax(y.detach(), dim=1)
        m = m.scatter(1, j[:, None], float('-inf'))
        S = S + y
        picks.append(j)
    return S, torch.stack(picks, 1)


class MLP(nn.Module):
    """Linear(dimIn, dimHid) - ReLU - Linear(dimHid, dimOut) (GSPAttack.py:120-130)."""

    def __init__(self, dimIn, dimHid, dimOut=1):
        super().__init__()
        self.dimIn, self.dimHid, self.dimOut = dimIn, dimHid, dimOut
        self.net = nn.Sequential(nn.Linear(dimIn, dimHid), nn.ReLU(), nn.Linear(dimHid, dimOut))

    def forward(self, x):
        return self.net(x)


class _PoisonedHop(torch.autograd.Function):
    """P = A_hat E for the poisoned normalised adjacency of a FactoredFakeGraph whose block was set from S.detach() (so d^-1/2 is a constant, as in
    the reference's torch.tensor(rowsum)).  Backward: dE = A_hat dP (A_hat symmetric) and, PGA's formula,
    dS[f, j] = dinv[U+f] dinv[R+j] (<dP[U+f], E[R+j]> + <dP[R+j], E[U+f]>)."""

    @staticmethod
    def forward(ctx, E, S, graph):
        E = E.contiguous()
        ctx.graph = graph
        ctx.save_for_backward(E)
        return graph.hop(E)

    @staticmethod
    def backward(ctx, gP):
        (E,), fg = ctx.saved_tensors, ctx.graph
        gP = gP.contiguous()
        gE = fg.hop(gP) if ctx.needs_input_grad[0] else None
        gS = None
        if ctx.needs_input_grad[1]:
            gS = torch.zeros(fg.F, fg.I, dtype=torch.float32, device=E.device)
            ops.sddmm_rows_dense(gP, E, fg.fake_rows, fg.Up, fg.I, out=gS)
            ops.sddmm_rows_dense(E, gP, fg.fake_rows, fg.Up, fg.I, out=gS)
            gS *= fg.dinv[fg.U:fg.Up, None] * fg.dinv[None, fg.Up:]
        return gE, gS, None


def poisoned_hop(E, S, graph):
    """One hop of the poisoned graph as an autograd node; graph.set_block(S.detach()) must have been called."""
    return _PoisonedHop.apply(E, S, graph)


class _DenseLayer(torch.autograd.Function):
    """leaky_relu((P + E) W1 + (P * E) W2) on ops.ngcf_dense_fwd / ops.ngcf_dense_bwd."""

    @staticmethod
    def forward(ctx, P, E, W1, W2):
        P, E = P.contiguous(), E.contiguous()
        Wcat = torch.cat([W1, W2], 0)
        out = ops.ngcf_dense_fwd(P, E, Wcat)
        ctx.save_for_backward(P, E, out, Wcat)
        return out

    @staticmethod
    def backward(ctx, g_out):
        P, E, out, Wcat = ctx.saved_tensors
        d = P.shape[1]
        gP, gE, gW = ops.ngcf_dense_bwd(g_out.contiguous(), out, P, E, Wcat)
        return gP, gE, gW[:d], gW[d:]


class _RealRowsBce(torch.autograd.Function):
    """sum_r rw[r] sum_i bce(<Pu[r], Pi[i]>, a[r, i]) over the real users through ops.bce_allpairs; the gradients the kernel returns enter autograd."""

    @staticmethod
    def forward(ctx, Pu, Pi, pos, pos_t, rw):
        loss, _, dPu, dPi = ops.bce_allpairs(Pu.contiguous(), Pi.contiguous(), pos, rw, eps=EPS, want_grad=True, pos_t=pos_t, check_range=False)
        ctx.save_for_backward(dPu, dPi)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dPu, dPi = ctx.saved_tensors
        return g * dPu, g * dPi, None, None, None


class NGCFProxy(nn.Module):
    """The repaired proxy (GSPAttack.py:132-223): nodes are users 0..R-1 then items R..R+I-1; real edges weigh 1, fake user f is connected to every
    item with weight S[f, i]; a layer is P = A_hat E, E' = leaky_relu((P + E) W1 + (P * E) W2); the output is the mean over the n_layers + 1
    tables.  Xavier-uniform tables and W; the MLP is Linear(2d, int(sqrt(I))) - ReLU - Linear(., 1)."""

    def __init__(self, ui_real, n_users, n_items, emb_size, n_layers, fakeUserNum, maliciousFeedbackNum, device=DEVICE):
        super().__init__()
        if emb_size not in ops.NGCF_DENSE_WIDTHS:
            raise ValueError('NGCFProxy: emb_size in %s' % (ops.NGCF_DENSE_WIDTHS,))
        self.user_num, self.item_num, self.latent_size, self.layers = int(n_users), int(n_items), int(emb_size), int(n_layers)
        self.fakeUserNum, self.maliciousFeedbackNum = int(fakeUserNum), int(maliciousFeedbackNum)
        self.mlp = MLP(2 * self.latent_size, int(math.sqrt(self.item_num)))
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({
            'user_emb': nn.Parameter(init(torch.empty(self.user_num + self.fakeUserNum, self.latent_size))),
            'item_emb': nn.Parameter(init(torch.empty(self.item_num, self.latent_size)))})
        w = dict()
        for i in range(self.layers):
            w['w1_' + str(i)] = nn.Parameter(init(torch.empty(self.latent_size, self.latent_size)))
            w['w2_' + str(i)] = nn.Parameter(init(torch.empty(self.latent_size, self.latent_size)))
        self.W = nn.ParameterDict(w)
        self.to(device)
        self.graph = FactoredFakeGraph(ui_real, self.user_num, self.fakeUserNum, self.item_num, device=device, emb_size=self.latent_size)

    def forward(self, S):
        """(Pu [R, d], Pi [I, d]) for the fake block S [F, I]; gradients reach the tables, every W and S."""
        fg = self.graph
        fg.set_block(S.detach())
        E = torch.cat([self.embedding_dict['user_emb'], self.embedding_dict['item_emb']], 0)
        acc = E
        for k in range(self.layers):
            E = _DenseLayer.apply(poisoned_hop(E, S, fg), E, self.W['w1_' + str(k)], self.W['w2_' + str(k)])
            acc = acc + E
        out = acc / (self.layers + 1)
        return out[:fg.Up], out[fg.Up:]

    def pair_logits(self, Pu_prev, Pi_prev):
        """x[f, i] = mlp(cat(Pu_prev[U+f], Pi_prev[i])) [F, I], one fake user at a time and recomputed in the backward: no F x I x H tensor exists."""
        def one(u_row):
            return self.mlp(torch.cat([u_row.expand(self.item_num, -1), Pi_prev], 1))[:, 0]
        return torch.stack([checkpoint(one, Pu_prev[self.user_num + f], use_reentrant=False) for f in range(self.fakeUserNum)], 0)

    def pair_logits_fused(self, Pu_prev, Pi_prev):
        """The same x [F, I] with the first layer split over its two inputs: A = E_f W1[:, :d]^T + b1 and B = E_i W1[:, d:]^T stay torch GEMMs (autograd
        carries the gradient to W1 and b1), the ReLU and the second layer over every pair run in ops.pair_mlp_logits_auto."""
        lin1, lin2, d = self.mlp.net[0], self.mlp.net[2], self.latent_size
        A = Pu_prev[self.user_num:] @ lin1.weight[:, :d].t() + lin1.bias
        B = Pi_prev @ lin1.weight[:, d:].t()
        return ops.pair_mlp_logits_auto(A, B, lin2.weight[0], lin2.bias)


class GSPAttack(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = False

    def __init__(self, arg, data, emb_size=64, n_layers=2):
        super().__init__(arg, data)
        self.itemP = np.array((self.interact.sum(0) / self.interact.sum()))[0]
        self.itemP[self.targetItem] = 0
        self.maliciousFeedbackNum = int(self.maliciousFeedbackNum)
        if self.maliciousFeedbackNum < 1 or self.maliciousFeedbackNum + len(self.targetItem) > self.itemNum:
            raise ValueError('GSPAttack: 1 <= maliciousFeedbackNum and maliciousFeedbackNum + targets <= items needed (k = %d, T = %d, I = %d)'
                             % (self.maliciousFeedbackNum, len(self.targetItem), self.itemNum))
        if self.fakeUserNum < 1:
            raise ValueError('GSPAttack: at least one fake user needed')
        self.attackForm = 'dataAttack'
        self.alpha = 1
        self.beta = 1
        self.batchSize = 128
        self.emb_size, self.n_layers = emb_size, n_layers
        self.ngcf = None                   # the NGCFProxy; built by the first posionDataAttack (or by _proxy()), so the constructor needs no GPU
        self.loss_log = []
        self.pick_log = []                 # the k picks per fake user of every epoch's Gumbel top-k
        self.first_dS = None               # dLoss/dS of the first epoch
        self.profile_route = 'composed'    # 'composed': the MLP per fake user and the Gumbel rounds in torch; 'fused': csrc/arl_profilegen.hip
        self.noise_source = 'torch'        # 'torch': self._noise((k, F, I)); 'hash': a counter hash of one seed per attack

    def _noise(self, shape):
        """Gumbel noise [k, F, I] on the device, drawn as F.gumbel_softmax draws it; a test replaces this method."""
        return -torch.empty(shape, dtype=torch.float32, device=DEVICE).exponential_().log()

    def _proxy(self):
        U, F, I = self.userNum, self.fakeUserNum, self.itemNum
        real = sp.csr_matrix(self.interact, dtype=np.float32)[:U]
        real.data[:] = 1.0                                                  # real edges have weight 1 (GSPAttack.py:157)
        ngcf = NGCFProxy(real, U, I, self.emb_size, self.n_layers, F, self.maliciousFeedbackNum, device=DEVICE)
        W = ngcf.graph.W                                                    # rows: R users (the fake ones empty), then I items; both CSR forms of the real edges
        nnz = int(real.nnz)
        self._pos = (W.rowptr[:U + 1].contiguous(), (W.col[:nnz] - (U + F)).contiguous())
        self._pos_t = ((W.rowptr[U + F:] - nnz).contiguous(), W.col[nnz:].contiguous())
        self._rw = ops.batch_mean_row_weights(U + F, I, self.batchSize, device=DEVICE)
        return ngcf

    def epoch_loss(self, ngcf, S):
        """alpha * L_per + beta * L_exPR for the fake block S (GSPAttack.py:62-83); returns (Loss, Pu, Pi)."""
        U = self.userNum
        Pu, Pi = ngcf(S)
        L_real = _RealRowsBce.apply(Pu[:U], Pi, self._pos, self._pos_t, self._rw[:U].contiguous())
        s = Pu[U:] @ Pi.t()                                                  # the fake users' F x I panel
        a = S.detach()
        bce = -(a * torch.log(torch.sigmoid(s) + EPS) + (1 - a) * torch.log(torch.sigmoid(-s) + EPS))
        L_per = L_real + (self._rw[U:, None] * bce).sum()
        tg = torch.as_tensor(self.targetItem, dtype=torch.long, device=s.device)
        L_exPR = (-torch.log(torch.sigmoid(s[:, tg]) + EPS)).mean()
        return self.alpha * L_per + self.beta * L_exPR, Pu, Pi

    def posionDataAttack(self):
        U, F, I, k = self.userNum, self.fakeUserNum, self.itemNum, self.maliciousFeedbackNum
        if self.profile_route not in ('composed', 'fused'):
            raise ValueError("GSPAttack: profile_route is 'composed' or 'fused', not %r" % (self.profile_route,))
        if self.noise_source not in ('torch', 'hash'):
            raise ValueError("GSPAttack: noise_source is 'torch' or 'hash', not %r" % (self.noise_source,))
        fused = self.profile_route == 'fused'
        hash_seed = random.getrandbits(63) if self.noise_source == 'hash' else None
        if self.ngcf is None:
            self.ngcf = self._proxy()
        ngcf = self.ngcf
        optimizer = Adam(ngcf.parameters(), lr=0.01)
        bestLoss, bestS = float('inf'), None
        with torch.no_grad():
            Pu_prev, Pi_prev = ngcf(torch.full((F, I), S_INIT, dtype=torch.float32, device=DEVICE))
        for epoch in range(self.Epoch):
            if not fused:
                x = ngcf.pair_logits(Pu_prev, Pi_prev)
                S, picks = gumbel_topk_relaxed(x, k, noise=self._noise((k, F, I)) if hash_seed is None else ops.gumbel_noise(hash_seed, epoch, k, F, I, DEVICE))
            else:
                x = ngcf.pair_logits_fused(Pu_prev, Pi_prev)
                if hash_seed is None:
                    S, picks = ops.gumbel_topk_auto(x, k, noise=self._noise((k, F, I)))
                else:
                    S, picks = ops.gumbel_topk_auto(x, k, seed=hash_seed, call=epoch)
            if epoch == 0:
                S.retain_grad()
            Loss, Pu, Pi = self.epoch_loss(ngcf, S)
            optimizer.zero_grad()
            Loss.backward()
            if epoch == 0:
                self.first_dS = S.grad.detach().clone()
            optimizer.step()
            Pu_prev, Pi_prev = Pu.detach(), Pi.detach()
            value = float(Loss.detach())
            self.loss_log.append(value)
            self.pick_log.append(picks.cpu())
            print('loss Value:{}'.format(value))
            if value < bestLoss:
                bestLoss, bestS = value, S.detach().clone()
            print('BiLevel epoch {} is over\n'.format(epoch + 1))
        if bestS is None:
            raise RuntimeError('GSPAttack: no epoch produced a finite loss')
        proj, _ = ops.topn_project_rows(bestS.contiguous(), k)
        proj[:, self.targetItem] = 1
        self.fakeUser = list(range(U, U + F))
        real = sp.csr_matrix(self.interact)[:U]
        self.interact = sp.vstack([real, sp.csr_matrix(proj.cpu().numpy())], format='csr', dtype=np.float32)
        return self.interact

"""RevAdv: "Revisiting Adversarially Learned Injection Attacks Against Recommender Systems" (Tang, Wen, Wang, RecSys'20).  The reference ships no such
attack; this class is written after the paper's description, not pinned to the authors' code, and is held to a float64 restatement
(tests/alsgrad_restatement.py).  It is the one attack of the library whose surrogate is the victim family the bilevel injection attacks are
formulated against: WRMF trained by ALS (recommender/iALS.py's model) on the real plus the fake data, with the adversarial loss differentiated
through the last ALS sweeps EXACTLY (arlib_amd/alsgrad.py: als_solve, the differentiable row solve on csrc/arl_als.hip).

Interface of the other data attacks: `RevAdv(arg, data)`, `posionDataAttack(recommender=None)` returns the scipy (U + F) x I matrix, the real rows
unchanged on top (as Black/_shilling.py's attacks return it); attributes fakeUser, W (the relaxed block), loss_log (L_adv of every outer epoch).

The surrogate is one CSR: the real rows with weight 1, plus F dense rows holding the relaxed block W in [0, 1]^(F x I), solved under alsgrad's
'relaxed' target rule; the item side is its transpose, val_item = val_user[perm], so autograd carries the permutation.  One outer epoch
(`outerEpoch` of them): rev_sweeps - rev_unroll sweeps without gradient, rev_unroll sweeps through als_solve,
    L_adv = -(1 / U) sum_{u real} sum_{t in targets} log softmax_i(x_u . y_i)[t]                          (util.loss.multinomial_nll)
backward to W, one Adam step, the clamp to [0, 1], the target columns back to 1.

Departures from the paper:
  1. The relaxation rule.  The paper trains the surrogate on the fake ratings as data; here a fake entry of weight w enters A_r with confidence
     alpha w and b_r with (1 + alpha) w, so that w = 1 is a stored entry, w = 0 an absent one, and everything between is differentiable.
  2. The fixed start of the surrogate.  Its initial tables are drawn once per attack from a generator seeded by rev_seed and are the same in every
     outer epoch, so the outer objective is a deterministic function of W (the paper re-initialises at random).
  3. Adam plus clamp.  W is stepped by torch's Adam at rev_lr and projected onto [0, 1], the target columns held at 1.
  4. The discretisation.  Every fake user ends with the targets plus its maliciousFeedbackNum - |targets| largest entries of W, ties broken by the
     lower item id (no sampling).
W starts at 0.5 x the profiles of F real users drawn with Python's `random` (the host stream the other attacks use), the targets at 1.

Size limit: the dense F x I block is held as CSR entries, so nnz_real + F I < 2^31 (and F x I floats of memory), as in PGA and GSPAttack; past it
the constructor raises."""
import numpy as np
import scipy.sparse as sp
import torch

from .._common import AttackBase
from ..Black._shilling import fake_block
from ... import als, alsgrad
from ...allpairs import transpose_positives
from ...multinomial import multinomial_nll
from ...util.sampler import sample_range


class RevAdv(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = False
    attackForm = 'dataAttack'
    rev_alpha = 10.0                  # confidence of a stored entry in the surrogate; arg.rev_alpha overrides
    rev_reg = 0.1                     # lambda of both tables; arg.rev_reg overrides
    rev_sweeps = 6                    # ALS sweeps of the surrogate per outer epoch; arg.rev_sweeps overrides
    rev_unroll = 2                    # the last this many sweeps are differentiated; arg.rev_unroll overrides
    rev_lr = 0.1                      # Adam's step on W; arg.rev_lr overrides
    rev_seed = 0                      # seed of the surrogate's initial tables; arg.rev_seed overrides
    rev_route = 'auto'                # route of the row solves and their adjoint: 'auto', 'fused' or 'composed'; arg.rev_route overrides
    rev_dtype = 'float32'             # 'float32' | 'float64' (composed route only); arg.rev_dtype overrides

    def __init__(self, arg, data):
        super().__init__(arg, data)
        self.attackForm = 'dataAttack'
        for k, conv in (('rev_alpha', float), ('rev_reg', float), ('rev_sweeps', int), ('rev_unroll', int), ('rev_lr', float), ('rev_seed', int),
                        ('rev_route', str), ('rev_dtype', str)):
            setattr(self, k, conv(getattr(arg, k, getattr(type(self), k))))
        self.emb_size = int(getattr(arg, 'emb_size', 64))
        if not self.rev_alpha >= 0.0 or not self.rev_reg > 0.0 or not 1 <= self.rev_unroll <= self.rev_sweeps or not self.rev_lr > 0.0 or (
                self.rev_route not in ('auto', 'fused', 'composed') or self.rev_dtype not in ('float32', 'float64')):
            raise ValueError("RevAdv: rev_alpha >= 0, rev_reg > 0, 1 <= rev_unroll <= rev_sweeps, rev_lr > 0, rev_route in ('auto', 'fused', 'composed'), "
                             "rev_dtype in ('float32', 'float64')")
        if self.rev_route == 'fused' and self.rev_dtype != 'float32':
            raise ValueError('RevAdv: the fused route is fp32')
        T = len(set(self.targetItem))
        if not T <= self.maliciousFeedbackNum <= self.itemNum:
            raise ValueError('RevAdv: |targets| <= maliciousFeedbackNum <= I needed (%d targets, budget %d, %d items)' % (T, self.maliciousFeedbackNum, self.itemNum))
        real = sp.csr_matrix(self.interact, dtype=np.float32)
        real.sum_duplicates(); real.eliminate_zeros(); real.sort_indices()
        if real.nnz + self.fakeUserNum * self.itemNum >= 2 ** 31:
            raise ValueError('RevAdv: the relaxed block is held dense: nnz_real + F * I = %d + %d * %d must stay below 2^31; use fewer fake users'
                             % (real.nnz, self.fakeUserNum, self.itemNum))
        self._real = real
        self.device = torch.device(getattr(arg, 'rev_device', 'cuda' if torch.cuda.is_available() else 'cpu'))
        self.W, self.fakeUser, self.loss_log = None, [], []
        self._plan = None

    # ------------------------------------------------------------------ the surrogate
    def _build(self):
        """The index arrays, fixed over the attack: the user-side CSR (real rows, then F dense rows), its transpose and both permutations; the
        surrogate's initial tables; the targets as the positives of every real user."""
        U, I, F, dev = self.userNum, self.itemNum, self.fakeUserNum, self.device
        dt = torch.float32 if self.rev_dtype == 'float32' else torch.float64
        m = self._real
        rowptr = np.concatenate([m.indptr.astype(np.int64), m.nnz + I * np.arange(1, F + 1, dtype=np.int64)]).astype(np.int32)
        col = np.concatenate([m.indices.astype(np.int32), np.tile(np.arange(I, dtype=np.int32), F)])
        rowptr, col = torch.from_numpy(rowptr).to(dev), torch.from_numpy(col).to(dev)
        tptr, trow, tperm = transpose_positives(rowptr, col, U + F, I)
        inv = torch.empty_like(tperm)
        inv[tperm.long()] = torch.arange(tperm.numel(), dtype=torch.int32, device=dev)
        g = torch.Generator().manual_seed(self.rev_seed)
        X0 = (0.1 * torch.randn(U + F, self.emb_size, generator=g, dtype=torch.float64)).to(dt).to(dev)
        Y0 = (0.1 * torch.randn(I, self.emb_size, generator=g, dtype=torch.float64)).to(dt).to(dev)
        targets = sorted(set(self.targetItem))
        T = len(targets)
        pos = (torch.arange(0, (U + 1) * T, T, dtype=torch.int32, device=dev), torch.tensor(targets * U, dtype=torch.int32, device=dev))
        self._plan = dict(user=(rowptr, col), item=(tptr, trow), tperm=tperm, inv=inv, X0=X0, Y0=Y0, pos=pos, ones=torch.ones(m.nnz, dtype=dt, device=dev),
                          targets=torch.tensor(targets, dtype=torch.long, device=dev), dtype=dt)
        return self._plan

    def initial_block(self):
        """W's start: 0.5 x the profiles of F real users drawn from Python's `random`, the targets at 1."""
        p = self._plan or self._build()
        users = sample_range(self.userNum, self.fakeUserNum)
        W = torch.from_numpy(0.5 * np.asarray(self._real[np.asarray(users, np.int64)].todense(), np.float64)).to(p['dtype']).to(self.device)
        W[:, p['targets']] = 1.0
        return W

    def outer_loss(self, W):
        """L_adv of the surrogate trained on the real rows plus the relaxed block W [F, I], differentiable in W through the last rev_unroll sweeps."""
        p = self._plan or self._build()
        (rowptr, col), (tptr, trow), tperm, inv = p['user'], p['item'], p['tperm'], p['inv']
        a, r, route = self.rev_alpha, self.rev_reg, self.rev_route
        val_u = torch.cat([p['ones'], W.reshape(-1)])
        val_i = val_u[tperm.long()]
        Y = p['Y0']
        with torch.no_grad():
            vu, vi = val_u.detach(), val_i.detach()
            for _ in range(self.rev_sweeps - self.rev_unroll):
                X = alsgrad.als_solve_rows_target(Y, als.gram(Y), (rowptr, col, vu), a, r, 'relaxed', route, check_range=False)
                Y = alsgrad.als_solve_rows_target(X, als.gram(X), (tptr, trow, vi), a, r, 'relaxed', route, check_range=False)
        for _ in range(self.rev_unroll):
            X = alsgrad.als_solve(Y, (rowptr, col, val_u), a, r, 'relaxed', route, transposed=(tptr, trow, tperm))
            Y = alsgrad.als_solve(X, (tptr, trow, val_i), a, r, 'relaxed', route, transposed=(rowptr, col, inv))
        nll = multinomial_nll(X[:self.userNum].contiguous(), Y, p['pos'], check_range=False)
        return nll.sum() / self.userNum

    def hypergradient(self, W):
        """(L_adv, dL_adv / dW [F, I]) at W."""
        W = W.detach().clone().requires_grad_(True)
        loss = self.outer_loss(W)
        g, = torch.autograd.grad(loss, W)
        return loss.detach(), g

    # ------------------------------------------------------------------ the attack
    def posionDataAttack(self, recommender=None):
        p = self._plan or self._build()
        W = self.initial_block().requires_grad_(True)
        opt = torch.optim.Adam([W], lr=self.rev_lr)
        for _ in range(self.outerEpoch):
            opt.zero_grad(set_to_none=True)
            loss = self.outer_loss(W)
            loss.backward()
            opt.step()
            with torch.no_grad():
                W.clamp_(0.0, 1.0)
                W[:, p['targets']] = 1.0
            self.loss_log.append(float(loss.detach()))
        self.W = W.detach()
        return self._fake_profiles()

    def _fake_profiles(self):
        """Every fake user: the targets plus its maliciousFeedbackNum - |targets| largest other entries of W, ties broken by the lower item id."""
        F, I = self.fakeUserNum, self.itemNum
        targets = sorted(set(self.targetItem))
        Wn = self.W.double().cpu().numpy()
        rest = np.setdiff1d(np.arange(I), targets)
        k = self.maliciousFeedbackNum - len(targets)
        rows = [rest[np.argsort(-Wn[f, rest], kind='stable')[:k]].tolist() + targets for f in range(F)]
        self.fakeUser = list(range(self.userNum, self.userNum + F))
        return sp.vstack([self.interact, fake_block(rows, F, I)])

"""GOAT (reference attack/Gray/GOAT.py): fake users from a GAN whose generator rates k candidate items per fake user -- items of one real user
that many other items are co-rated with (I_s, I_f), filled up with random draws -- and whose outputs are projected to the top
maliciousFeedbackNum items of each row, the targets set to 1 first.

Interface and streams as in the reference: `GOAT(arg, data)`, `posionDataAttack(epoch1=20, epoch2=20, O_u=0.01, O_g=0.1, O_i=0.02)`,
`itemSample(k, O_u, O_g, O_i)` with its three lists, attributes G, D, D_r = None, k, t, itemIntNum (a list of floats), BiLevelOptimizationEpoch = 50.
What the reference cannot do at a million users is done natively:
  * itemIntNum, the co-rating degree, comes from arlib_amd.corating (an LDS bitmap per item instead of the I x I product; the scipy expression
    past the kernel's limit).  `item_itemInteract` is still there, evaluated on first access: the attack never reads it.
  * itemSample runs in the library (arl_goat_item_sample) on Python's own MT19937 state: the same values and the same consumption of `random`
    as the reference's loop, without a dense row per draw or a set of all items per fake user.  That is exact while the fill draws' set iterates
    in ascending order, k + len(targets) <= 0.4 I; past that bound the reference's own expression is evaluated in Python (item_sample_python).
  * the final projection is ops.topn_project_rows over row chunks (the project's pinned tie rule: equal values go to the lower column).
The GAN itself (k -> 64 -> 32 -> 16 k MLPs on F rows) stays composed from torch ops on the device, stepped by util.optim.Adam: G and D are built
on the CPU in the reference's order (so their initial parameters match bit for bit), Z is drawn from torch's CPU generator.  G runs in fp32 as in
the reference; D's step is evaluated in float64 on its fp32 parameters (d_loss says why).

Kept quirks: ONE real user per itemSample call, shared by all fake rows (realUser is reset per call, not per row); the
`elif` order of the walk (an item that qualifies for I_s goes to I_f once I_s is full); `ratingNumThreshold / 3` is a float division;
int(0.3 k) + int(0.7 k) can be k - 1, so the fill draw is the normal case; in a short run G's outputs exceed 1 and the cut falls among the
targets' ties.  Not kept: k == 0 (the reference's O_g branch, which redefines k inside the loop) raises ValueError, and a data set without a
user of O_u * I items raises ValueError where the reference never returns.
"""
import random

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from .._common import AttackBase
from ...util.sampler import MTState, sample_range
from ...util.optim import Adam
from ... import _lib, corating, ops

DEVICE = 'cuda'
PROJECT_CHUNK_BYTES = 1 << 30          # M, out and scratch of one topn_project_rows call stay under this each


class MLP(nn.Module):
    """GOAT.py:138-153: net.layer_i Linear, net.bias_i LeakyReLU(0.2) or Sigmoid."""

    def __init__(self, inputSize, hiddenSize, sigmoidFunc=False):
        super(MLP, self).__init__()
        self.net = nn.Sequential()
        for i in range(len(hiddenSize)):
            self.net.add_module('layer_{}'.format(i), nn.Linear(inputSize if i == 0 else hiddenSize[i - 1], hiddenSize[i]))
            self.net.add_module('bias_{}'.format(i), nn.Sigmoid() if sigmoidFunc else nn.LeakyReLU(0.2))

    def forward(self, x):
        return self.net(x)


class Encoder(nn.Module):
    """The generator (GOAT.py:156-170): R = G_r(flatten(G_e(x).reshape(F, k, 16) @ (G_l(x)^T G_l(x))))."""

    def __init__(self, k):
        self.k = k
        super(Encoder, self).__init__()
        self.G_e = MLP(k, [64, 32, 16 * k])
        self.G_l = MLP(k, [64, 32, 16])
        self.G_r = MLP(k * 16, [k])

    def forward(self, x):
        L_t = self.G_l(x)
        H = self.G_e(x).reshape(x.shape[0], self.k, 16)
        L = L_t.T @ L_t
        R_t1 = torch.bmm(H, L.unsqueeze(0).repeat((x.shape[0], 1, 1)))
        return self.G_r(R_t1.view((-1, R_t1.shape[1] * R_t1.shape[2])))


class Decoder(nn.Module):
    """The discriminator (GOAT.py:173-179): k -> 64 -> 32 -> 16 -> 1, a Sigmoid after every layer."""

    def __init__(self, k):
        super(Decoder, self).__init__()
        self.D_r = MLP(k, [64, 32, 16, 1], sigmoidFunc=True)

    def forward(self, x):
        return self.D_r(x)


# ---------------------------------------------------------------------------------------------------- itemSample
def native_sampling_exact(k, n_targets, n_items):
    """True while arl_goat_item_sample restates the reference exactly: the set of the fill draws iterates in ascending order while the removed
    ids are at most 0.4 I (CPython's table of a set of n small ints is a power of two above 5 n / 3: larger than its largest member)."""
    return k >= 1 and (k + n_targets) <= 0.4 * n_items


class SampleData:
    """What itemSample reads, checked once: the interaction CSR (int64 rowptr, int32 items ascending per user), itemIntNum as float64, the targets
    as int32, and the largest user degree.  GOAT builds one in its constructor (the matrix never changes afterwards), so the 2 001 calls of an
    attack do not walk the 32 M ids of a large graph again; the free functions below also take the six raw arguments and build one per call."""

    def __init__(self, rowptr, items, n_users, n_items, int_num, targets):
        n_users, n_items = int(n_users), int(n_items)
        if n_users < 1 or n_items < 1:
            raise ValueError('GOAT.itemSample: %d x %d interactions' % (n_users, n_items))
        rowptr, items = np.ascontiguousarray(rowptr, np.int64), np.ascontiguousarray(items, np.int32)
        int_num, targets = np.ascontiguousarray(int_num, np.float64), np.ascontiguousarray(targets, np.int32).reshape(-1)
        if len(rowptr) != n_users + 1 or len(int_num) != n_items or rowptr[0] != 0 or rowptr[-1] != len(items):
            raise ValueError('GOAT.itemSample: rowptr [U + 1], items [nnz], int_num [I] needed')
        if targets.size and (int(targets.min()) < 0 or int(targets.max()) >= n_items):
            raise ValueError('GOAT.itemSample: target item outside [0, %d)' % n_items)
        if items.size and (int(items.min()) < 0 or int(items.max()) >= n_items):
            raise ValueError('GOAT.itemSample: item id outside [0, %d)' % n_items)
        deg = np.diff(rowptr)
        if deg.min() < 0:
            raise ValueError('GOAT.itemSample: rowptr must not decrease')
        self.rowptr, self.items, self.n_users, self.n_items, self.int_num, self.targets = rowptr, items, n_users, n_items, int_num, targets
        self.max_degree = int(deg.max())


def _sample_args(args):
    """(SampleData, n_fake, k, O_u * I) of a call (data, n_fake, k, O_u, O_i) or (rowptr, items, n_users, n_items, int_num, targets, n_fake, k, O_u,
    O_i); the per-call checks: k, and that some user has O_u * I items."""
    data, rest = (args[0], args[1:]) if isinstance(args[0], SampleData) else (SampleData(*args[:6]), args[6:])
    n_fake, k, O_u, O_i = rest
    k, n_fake = int(k), int(n_fake)
    if k == 0:
        raise ValueError('GOAT.itemSample: k == 0 (the reference\'s O_g branch) is not supported')
    if k < 0 or n_fake < 0:
        raise ValueError('GOAT.itemSample: k = %d, %d fake users' % (k, n_fake))
    min_items = O_u * data.n_items
    if n_fake and data.max_degree < min_items:
        raise ValueError('GOAT.itemSample: no user has O_u * I = %g items (the reference would draw forever)' % min_items)
    return data, n_fake, k, min_items, O_i


def item_sample_native(*args):
    """One itemSample call in the library on Python's `random` state: (data, n_fake, k, O_u, O_i) with a SampleData, or the six raw arguments in
    its place.  Returns (I_s int32 [F, int(0.3 k)], I_f int32 [F, k - int(0.3 k)], real uint8 [F, k], the real user's id).  ArlError
    (ARL_E_RANGE) past native_sampling_exact."""
    d, F, k, min_items, O_i = _sample_args(args)
    L, vp = _lib.lib(), lambda a: a.ctypes.data
    ks = int(k * 0.3)
    out_s, out_f = np.empty((F, max(ks, 1)), np.int32), np.empty((F, max(k - ks, 1)), np.int32)
    real, user = np.empty((F, k), np.uint8), np.full(1, -1, np.int32)
    scratch = np.empty(L.arl_goat_item_sample_scratch_words(d.n_items, k, len(d.targets)), np.int32)
    mt = MTState.from_python()
    _lib.check(L.arl_goat_item_sample(vp(mt.words), vp(d.rowptr), vp(d.items), d.n_users, d.n_items, vp(d.int_num), vp(d.targets), len(d.targets), F, k,
                                      float(min_items), int(O_i * d.n_users), vp(out_s), vp(out_f), vp(real), vp(user), vp(scratch)), 'arl_goat_item_sample')
    mt.to_python()
    return out_s[:, :ks], out_f[:, :k - ks], real, int(user[0])


def item_sample_python(*args):
    """The reference's loop (GOAT.py:105-135) on the CSR, with its own pool expression: the set is built as the reference builds it, turned into
    the tuple CPython 3.10's random.sample would make of it, and indexed with sample_range -- exact for any k, also on Python >= 3.11 where
    random.sample of a set raises.  The route past native_sampling_exact.  Same arguments and returns as item_sample_native."""
    d, F, k, min_items, O_i = _sample_args(args)
    rowptr, items, U, I, int_num, targets = d.rowptr, d.items, d.n_users, d.n_items, d.int_num, d.targets
    thr, ks, kf = int(O_i * U), int(k * 0.3), int(k * 0.7)
    tg = targets.tolist()
    out_s, out_f, real = np.empty((F, ks), np.int32), np.empty((F, k - ks), np.int32), np.empty((F, k), np.uint8)
    user, have, mine = -1, 0.0, np.zeros(0, np.int32)
    for f in range(F):
        I_s, I_f = [], []
        while have < min_items:
            user = random.randint(0, U - 1)
            mine = np.sort(items[rowptr[user]:rowptr[user + 1]])
            have = float(len(mine))
        for j in mine.tolist():
            if int_num[j] > thr and len(I_s) < ks:
                I_s.append(j)
            elif int_num[j] > thr / 3 and len(I_f) < kf:
                I_f.append(j)
        while len(I_s) < ks:
            pool = tuple(set(list(range(I))) - set(tg) - set(I_s) - set(I_f))
            I_s += [pool[i] for i in sample_range(len(pool), ks - len(I_s))]
        while len(I_f) + len(I_s) < k:
            pool = tuple(set(list(range(I))) - set(tg) - set(I_s) - set(I_f))
            I_f += [pool[i] for i in sample_range(len(pool), k - len(I_f) - len(I_s))]
        out_s[f], out_f[f] = I_s, I_f
        real[f] = np.isin(np.asarray(I_s + I_f, np.int32), mine)
    return out_s, out_f, real, user


def item_sample(*args):
    """item_sample_native where it is exact, item_sample_python otherwise."""
    d, F, k, _, O_i = _sample_args(args)
    fn = item_sample_native if native_sampling_exact(k, len(d.targets), d.n_items) else item_sample_python
    return fn(d, *args[-4:])


# ---------------------------------------------------------------------------------------------------- the GAN's steps
def d_loss(G, D, Z, real):
    """(D(G(Z)) - D(real)).mean() with D evaluated in float64 on its fp32 parameters (the gradients arrive in fp32).  loss1 is the difference of two
    nearly equal means of sigmoid outputs: evaluated in fp32, as the reference does, its value and D's bias gradients are off by 1e-5 to 1.5e-4 of
    themselves from the rounding of the outputs alone (tests/test_gpu_goat.py measures it on the reference's first step).  D is k -> 64 -> 32 -> 16
    -> 1 on 2 F rows, so float64 costs nothing that shows."""
    with torch.no_grad():
        Y = G(Z)
    P = {n: p.double() for n, p in D.named_parameters()}
    return (torch.func.functional_call(D, P, (Y.double(),)) - torch.func.functional_call(D, P, (real.double(),))).mean()


def d_step(G, D, opt_D, Z, real):
    """loss1 = (D(G(Z)) - D(real)).mean(), D stepped.  The reference's backward also reaches G, but optimize_G.zero_grad() precedes every G
    backward, so those gradients are never used: G runs without a graph."""
    loss = d_loss(G, D, Z, real)
    opt_D.zero_grad()
    loss.backward()
    opt_D.step()
    return loss.detach()


def g_loss(G, D, Z, real, k):
    Y = G(Z)
    return (-D(Y) + 0.01 * (1 / k) * torch.linalg.norm(Y - real)).mean()


def g_step(G, D, opt_G, Z, real, k):
    """loss2 = (-D(Y) + 0.01 / k * |Y - real|_F).mean(), Y = G(Z), G stepped (D's gradients of this backward are zeroed before D's next one)."""
    loss = g_loss(G, D, Z, real, k)
    opt_G.zero_grad()
    loss.backward(inputs=list(G.parameters()))
    opt_G.step()
    return loss.detach()


@torch.no_grad()
def project_rows(Y, I_s, I_f, targets, n_items, n):
    """The reference's dense rule per fake row (GOAT.py:89-93, 98-103) in row chunks: a zero row of n_items entries, Y[f] at the row's candidates,
    1 at the targets, then the ids of its n largest entries (ops.topn_project_rows: ties go to the lower column).  Returns int64 [F, n], ascending."""
    F = Y.shape[0]
    cand = torch.from_numpy(np.concatenate([I_s, I_f], 1).astype(np.int64)).to(Y.device)
    tg = torch.as_tensor(targets, dtype=torch.int64, device=Y.device)
    step = max(1, PROJECT_CHUNK_BYTES // (4 * n_items))
    cols = []
    for r0 in range(0, F, step):
        M = torch.zeros(min(step, F - r0), n_items, dtype=torch.float32, device=Y.device)
        M.scatter_(1, cand[r0:r0 + step], Y[r0:r0 + step])
        M[:, tg] = 1
        cols.append(ops.topn_project_rows(M, n)[1].cpu().numpy().astype(np.int64))
    return np.sort(np.concatenate(cols, 0), 1) if cols else np.zeros((0, n), np.int64)


class GOAT(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = False
    attackForm = 'dataAttack'

    def __init__(self, arg, data):
        super().__init__(arg, data)
        self.targetSize = arg.targetSize
        self.G = None
        self.D = None
        self.D_r = None
        ui = sp.csr_matrix(self.interact)
        ui.sum_duplicates()
        ui.sort_indices()
        if ui.nnz and not (ui.data == 1).all():
            raise ValueError('GOAT: a 0/1 interaction matrix is needed (realUser.sum() is read as the number of items)')
        int_num = self.co_rating(ui)
        self.itemIntNum = int_num.tolist()
        self._sample_data = SampleData(ui.indptr, ui.indices, self.userNum, self.itemNum, int_num, self.targetItem)       # checked here, once
        self._item_item = None
        self.attackForm = 'dataAttack'
        self.recommenderGradientRequired = False
        self.recommenderModelRequired = False
        self.BiLevelOptimizationEpoch = 50
        self.loss_log = []                 # device scalars: loss1 of every D step and loss2 of every G step, in order
        self.real_users = []               # the real user of every itemSample call, in order

    @staticmethod
    def co_rating(interact):
        """itemIntNum as a float64 array: the kernel where the catalogue fits its bitmap, the reference's scipy expression otherwise."""
        ui = sp.csr_matrix(interact)
        U, I = ui.shape
        if corating.corating_degree_supported(I):
            return corating.corating_degree(ui.indptr, ui.indices, U, I, device=DEVICE).cpu().numpy().astype(np.float64)
        return corating.corating_degree_host(ui)

    @property
    def item_itemInteract(self):
        """interact.T @ interact with every stored entry set to 1 (GOAT.py:37-38), evaluated on first access."""
        if self._item_item is None:
            m = (self.interact.T @ self.interact).tocsr()
            m.data[m.data > 0] = 1
            self._item_item = m
        return self._item_item

    # ------------------------------------------------------------------ sampling
    def _sample(self, k, O_u, O_i):
        I_s, I_f, real, user = item_sample(self._sample_data, self.fakeUserNum, k, O_u, O_i)
        self.real_users.append(user)
        return I_s, I_f, real

    def itemSample(self, k, O_u, O_g, O_i):
        """The reference's three lists: I_s and I_f (a list of item ids per fake user) and realUserList (per fake user, the real user's row at the
        k candidates, float64).  O_g is read by the k == 0 branch only, which raises here."""
        I_s, I_f, real = self._sample(k, O_u, O_i)
        return I_s.tolist(), I_f.tolist(), list(real.astype(np.float64))

    def _draw(self, k, O_u, O_i):
        """One step's inputs in the reference's order: the sample from Python's `random`, then Z from torch's CPU generator."""
        I_s, I_f, real = self._sample(k, O_u, O_i)
        Z = torch.randn(real.shape)
        return I_s, I_f, torch.from_numpy(real).to(DEVICE, torch.float32), Z.to(DEVICE)

    # ------------------------------------------------------------------ attack
    def posionDataAttack(self, epoch1=20, epoch2=20, O_u=0.01, O_g=0.1, O_i=0.02):
        if self.G is None:
            k = self.maliciousFeedbackNum
            if k == 0:
                raise ValueError('GOAT: maliciousFeedbackNum == 0 (the reference\'s O_g branch) is not supported')
            self.k = k
            self.G = Encoder(k).to(DEVICE)
            self.D = Decoder(k).to(DEVICE)
            optimize_G = Adam(self.G.parameters(), lr=0.005)
            optimize_D = Adam(self.D.parameters(), lr=0.005)
            for i in range(self.BiLevelOptimizationEpoch):
                self.G.eval()
                self.D.train()
                for k1 in range(epoch1):
                    _, _, real, Z = self._draw(k, O_u, O_i)
                    self.loss_log.append(d_step(self.G, self.D, optimize_D, Z, real))
                self.D.eval()
                self.G.train()
                for k2 in range(epoch2):
                    _, _, real, Z = self._draw(k, O_u, O_i)
                    self.loss_log.append(g_step(self.G, self.D, optimize_G, Z, real, self.k))
        return self._fake_profiles(O_u, O_i)

    @torch.no_grad()
    def _fake_profiles(self, O_u, O_i):
        """The trained G on one more sample: its k outputs at the row's candidates, the targets at 1, then the top maliciousFeedbackNum entries of
        every dense row become 1 (GOAT.py:83-96), in row chunks."""
        self.G.eval()
        I_s, I_f, real, Z = self._draw(self.k, O_u, O_i)
        Y = self.G(Z)
        F, I, n = self.fakeUserNum, self.itemNum, int(self.maliciousFeedbackNum)
        self.last_sample, self.last_Y = (I_s, I_f), Y
        cols = project_rows(Y, I_s, I_f, self.targetItem, I, n)
        fakeRat = sp.csr_matrix((np.ones(F * n, np.float32), cols.reshape(-1), np.arange(F + 1, dtype=np.int64) * n), shape=(F, I), dtype=np.float32)
        # the reference keeps the dense F x I tensor here; this is the same matrix, sparse (self.t.to_dense() is the reference's)
        self.t = torch.sparse_coo_tensor(np.stack([np.repeat(np.arange(F), n), cols.reshape(-1)]), torch.ones(F * n), (F, I))
        return sp.vstack([self.interact, fakeRat])

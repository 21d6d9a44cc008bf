"""AUSH (reference attack/Gray/AUSH.py): fake users from a GAN over a template of real users' ratings on I // 5 random items plus the targets.

Interface and streams as in the reference: `AUSH(arg, data)`, `posionDataAttack(epoch1=25, epoch2=25)`, attributes G, D, selectItem, fakeUser,
fakeRat and BiLevelOptimizationEpoch = 50; G and D are built on the CPU in the reference's order (so their initial parameters match bit for
bit) and trained on the first call only.  selectItem and every step's userSet come from Python's `random` (sampler.sample_range, the same
values and consumption as the reference's `random.sample` of a set), the template masks from numpy's global RandomState, drawn as the
reference draws them.  The template itself, the GAN's steps and the final thresholding run on the arl_gan_* kernels (attack/Gray/_gan.py).

The template keeps the reference's quirk (AUSH.py:64-72): for a stored (r, c) of interact[userSet] with c selected, column j = the position
of c and value interact[r, j] * mask[r, j] -- local row r and position j read as a user and an item id.

template_rng='device' (opt-in) draws the masks inside the template kernel from a counter hash of (template_seed, call, row, item) instead:
the same Bernoulli(itemP) distribution, another stream, and no F x I host draw per step (which dominates at a million users).
"""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn as nn

from .._common import AttackBase
from ..Black._shilling import remaining_ids
from ...util.sampler import sample_range
from ...util.optim import Adam
from ... import ops
from . import _gan

DEVICE = 'cuda'


class Generator(nn.Module):
    """MLP of the reference (AUSH.py:152-168): net.layer_0 Linear(S, S), net.bias_0 ReLU, net.layer_1 Linear(S, S), net.bias_1 Sigmoid."""

    def __init__(self, size, layer=2):
        self.layer = layer
        super(Generator, self).__init__()
        self.net = nn.Sequential()
        for i in range(self.layer):
            self.net.add_module('layer_{}'.format(i), nn.Linear(size, size))
            self.net.add_module('bias_{}'.format(i), nn.ReLU() if i != self.layer - 1 else nn.Sigmoid())

    def forward(self, x):
        return self.net(x)


class Discriminator(nn.Module):
    """Linear(S, 1) -> Sigmoid (AUSH.py:171-181)."""

    def __init__(self, size):
        super(Discriminator, self).__init__()
        self.net = nn.Sequential(nn.Linear(size, 1), nn.Sigmoid())

    def forward(self, x):
        return self.net(x)


def draw_masks(itemP, selectItem, F, rows_per_draw=256):
    """`np.array([np.random.binomial(1, itemP)[selectItem] for i in range(F)])` (AUSH.py:61-62) in (rows_per_draw, I) draws: numpy's legacy
    binomial walks the broadcast array in C order with the same per-element generator, so the stream and the values are those of the F row
    calls (tests/test_shilling_cpu.py checks it), and host memory stays at rows_per_draw x I draws.  Returns uint8 [F, S]."""
    sel = np.asarray(selectItem, np.int64)
    out = np.empty((F, len(sel)), np.uint8)
    for r0 in range(0, F, rows_per_draw):
        n = min(rows_per_draw, F - r0)
        out[r0:r0 + n] = np.random.binomial(1, itemP, size=(n, len(itemP)))[:, sel]
    return out


def host_template(interact, userSet, mask, pos, S=None):
    """The reference's template (AUSH.py:63-72) as the scipy CSR it builds, vectorised: for every stored (r, c) of interact[userSet] with
    pos[c] >= 0, column j = pos[c] and value interact[r, j] * mask[r, j]; explicit zeros kept.  mask: [F, S] array, or a function
    (rows, cols) -> mask values (then S is given)."""
    F = len(userSet)
    S = mask.shape[1] if S is None else S
    r, c = interact[userSet, :].nonzero()
    j = pos[c]
    keep = j >= 0
    r, j = r[keep], j[keep]
    m = mask(r, j) if callable(mask) else mask[r, j]
    vals = np.asarray(interact[r, j]).ravel() * m if len(r) else np.zeros(0)
    return sp.csr_matrix((vals, (r, j)), shape=(F, S), dtype=np.float32)


class AUSH(AttackBase):
    recommenderGradientRequired = False
    recommenderModelRequired = False
    attackForm = 'dataAttack'

    def __init__(self, arg, data, template_rng='host', template_seed=0):
        super().__init__(arg, data)
        if template_rng not in ('host', 'device'):
            raise ValueError("AUSH: template_rng is 'host' (the reference's numpy stream) or 'device' (in-kernel counter hash)")
        self.targetSize = arg.targetSize
        self.G = None
        self.D = None
        self.itemP = np.array((self.interact.sum(0) / self.interact.sum()))[0]
        self.itemP[self.targetItem] = 0
        self.attackForm = 'dataAttack'
        self.BiLevelOptimizationEpoch = 50
        self.template_rng, self.template_seed, self._calls = template_rng, int(template_seed), 0
        self.loss_log = []                 # device scalars: loss1 of every D step and loss2 of every G step, in order

    # ------------------------------------------------------------------ template
    def _device_state(self):
        if getattr(self, '_dev', None) is None:
            ui = sp.csr_matrix(self.interact, dtype=np.float32)
            if not ui.has_sorted_indices:
                ui = ui.sorted_indices()
            t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEVICE)
            pos = np.full(self.itemNum, -1, np.int32)
            pos[np.asarray(self.selectItem, np.int64)] = np.arange(len(self.selectItem), dtype=np.int32)
            self._dev = dict(rowptr=t(ui.indptr, np.int64), col=t(ui.indices, np.int32), val=t(ui.data, np.float32), pos=t(pos, np.int32),
                             pos_host=pos, items=t(self.selectItem, np.int32), item_p=t(self.itemP, np.float32))
        return self._dev

    def _template(self):
        """One step's template: userSet from Python's random, masks from numpy's global stream (or the counter hash), built by the kernel."""
        dv = self._device_state()
        userSet = sample_range(self.userNum, self.fakeUserNum)
        us = torch.from_numpy(userSet.astype(np.int32)).to(DEVICE)
        if self.template_rng == 'host':
            mask = draw_masks(self.itemP, self.selectItem, self.fakeUserNum)
            if ops.gan_template_supported(self.fakeUserNum, len(self.selectItem)):
                rp, col, val = ops.gan_template(us, dv['rowptr'], dv['col'], dv['val'], dv['pos'], dv['items'], mask=torch.from_numpy(mask).to(DEVICE))
            else:
                rp, col, val = self._host_template(userSet, mask)
        elif ops.gan_template_supported(self.fakeUserNum, len(self.selectItem)):
            rp, col, val = ops.gan_template(us, dv['rowptr'], dv['col'], dv['val'], dv['pos'], dv['items'], item_p=dv['item_p'],
                                            seed=self.template_seed, call=self._calls)
        else:
            sel, call = np.asarray(self.selectItem, np.int64), self._calls
            keep = lambda r, j: ops.gan_hash_keep(r, sel[j], self.itemP, self.template_seed, call).astype(np.float32)
            rp, col, val = self._host_template(userSet, keep)
        self._calls += 1
        return _gan.Template(rp, col, val, len(self.selectItem))

    def _host_template(self, userSet, mask):
        """The template past the kernel's limits: host_template (the same entries, columns ascending per row) moved to the device."""
        t = host_template(self.interact, userSet, mask, self._dev['pos_host'].astype(np.int64), S=len(self.selectItem))
        d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(DEVICE)
        return d(t.indptr, np.int64), d(t.indices, np.int32), d(t.data, np.float32)

    # ------------------------------------------------------------------ attack
    def fused(self):
        return ops.gan_supported(self.fakeUserNum, len(self.selectItem))

    def posionDataAttack(self, epoch1=25, epoch2=25):
        if self.G is None:
            pool = remaining_ids(self.itemNum, self.targetItem)
            self.selectItem = pool[sample_range(len(pool), self.itemNum // 5)].tolist() + self.targetItem
            S, T = len(self.selectItem), len(self.targetItem)
            G = Generator(S)
            D = Discriminator(S)
            G, D = G.to(DEVICE), D.to(DEVICE)
            optimize_G = Adam(G.parameters(), lr=0.005)
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
                    self.loss_log.append(_gan.g_step(G, D, optimize_G, self._template(), T, fused))
            self.G = G
            self.D = D
        return self._fake_profiles()

    def _fake_profiles(self):
        """The trained G on one more template, thresholded at 0.1, the targets appended to every fake row (AUSH.py:116-141)."""
        self.G.eval()
        tpl = self._template()
        Y, rowptr, col = _gan.generate(self.G, tpl, self.fused())
        self.fakeUser = list(range(self.userNum, self.userNum + self.fakeUserNum))
        F = self.fakeUserNum
        rowptr, col = rowptr.cpu().numpy(), col.cpu().numpy().astype(np.int64)
        if F:
            last = np.zeros(len(self.selectItem), np.float32)
            last[col[rowptr[F - 1]:rowptr[F]]] = 1
            self.fakeRat = torch.from_numpy(last)
        sel = np.asarray(self.selectItem, np.int64)
        counts = np.diff(rowptr)
        T = len(self.targetItem)
        rows = np.concatenate([np.repeat(np.arange(F), counts), np.repeat(np.arange(F), T)])
        cols = np.concatenate([sel[col], np.tile(np.asarray(self.targetItem, np.int64), F)])
        fakeRat = sp.csr_matrix((np.ones(len(cols), np.float32), (rows, cols)), shape=(F, self.itemNum), dtype=np.float32)
        return sp.vstack([self.interact, fakeRat])

#!/usr/bin/env python3
"""Golden vectors for the shilling attacks: runs the reference's own attack/Black/RandomAttack.py, BandwagonAttack.py and attack/Gray/AUSH.py
on the CPU (ml-100k, seedSet(2018)) with the shims of gen_golden.py, and writes g30_shilling.npz (data only).

Every attack is built with maliciousUserSize = 0.01 (9 fake users), maliciousFeedbackSize = 0 and 5 unpopular targets, after seedSet(2018)
and a fresh DataLoader; `random.seed(11); np.random.seed(11); torch.manual_seed(11)` precede each posionDataAttack call.

  g30_shilling.npz
    rand_row / rand_col / rand_val, band_*       the fake blocks (rows U.. of the result) as COO arrays in CSR order
    rand_state_sha / band_state_sha              SHA-256 of repr(random.getstate()) after posionDataAttack
    rand_targets / band_targets / aush_targets   internal target ids
    aush_select                                  selectItem
    aush_init_sha__<p>, aush_init_row__<p>       digest and first row of each initial parameter (G.net.layer_0.weight, ... D.net.0.bias)
    aush_tpl_sha                                 [2500] SHA-256 (hex) of each training step's template: rows, cols (int32) and values
                                                 (float32) of the coalesced sparse tensor handed to G, in step order
    aush_loss                                    [2500] loss1 of each D step / loss2 of each G step in order (25 D, 25 G, 50 times)
    aush_loss_t1                                 the same run at one torch thread (the spread of the reference's own fp32 arithmetic)
    aush_ckpt_steps, aush_ckpt__<p>              rows 0, 7 and the last of W1 / W2 (and all of b1, b2, wD, bD) after those G steps
    aush_ckpt_t1__<p>                            the same at one torch thread
    aush_final_Y                                 [9, 287] the final G outputs (S = 282 + 5 on the training split);  aush_row / aush_col / aush_val: the fake block

Usage:  python tests/golden/gen_golden_shilling.py
"""
import contextlib
import hashlib
import io
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
from util.tool import seedSet                          # noqa: E402
from util.DataLoader import DataLoader                 # noqa: E402
import attack.Gray.AUSH as RA                          # noqa: E402
from attack.Black.RandomAttack import RandomAttack     # noqa: E402
from attack.Black.BandwagonAttack import BandwagonAttack  # noqa: E402

PARAMS = ('G.net.layer_0.weight', 'G.net.layer_0.bias', 'G.net.layer_1.weight', 'G.net.layer_1.bias', 'D.net.0.weight', 'D.net.0.bias')
CKPT = (50, 625, 1250, 2500)          # 1-based counts of optimiser steps (D and G together) after which parameters are sampled


def attack_args(name, category):
    return G._attack_args(attackCategory=category, attackModelName=name, maliciousUserSize=0.01, maliciousFeedbackSize=0, targetSize=5)


def sha(*arrs):
    h = hashlib.sha256()
    for a in arrs:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fresh_data():
    """seedSet(2018) and a fresh DataLoader; the reference's target cache file is removed so that every build draws its targets (as the
    product does where no cache exists)."""
    os.makedirs('data/clean/ml-100k', exist_ok=True)
    cache = 'data/clean/ml-100k/targetItem_unpopular_5.txt'
    if os.path.exists(cache):
        os.remove(cache)
    seedSet(2018)
    return DataLoader(G.rec_args())


def reseed():
    random.seed(11); np.random.seed(11); torch.manual_seed(11)


def block(res, U):
    f = res.tocsr()[U:]
    f.sort_indices()
    r = np.repeat(np.arange(f.shape[0]), np.diff(f.indptr)).astype(np.int32)
    return r, f.indices.astype(np.int32), f.data.astype(np.float32)


def shilling(out):
    for cls, tag in ((RandomAttack, 'rand'), (BandwagonAttack, 'band')):
        data = fresh_data()
        atk = cls(attack_args(cls.__name__, 'Black'), data)
        reseed()
        res = atk.posionDataAttack()
        out[tag + '_row'], out[tag + '_col'], out[tag + '_val'] = block(res, atk.userNum)
        out[tag + '_state_sha'] = np.array(sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8)))
        out[tag + '_targets'] = np.array(atk.targetItem, np.int32)


def params_of(atk_G, atk_D):
    return dict(zip(PARAMS, [p for p in atk_G.parameters()] + [p for p in atk_D.parameters()]))


def aush(threads):
    torch.set_num_threads(threads)
    data = fresh_data()
    atk = RA.AUSH(attack_args('AUSH', 'Gray'), data)
    cap = dict(tpl=[], loss=[], ckpt={}, init=None, final_Y=[])
    orig_fwd, orig_backward, orig_step = RA.Generator.forward, torch.Tensor.backward, torch.optim.Adam.step
    orig_init = RA.Discriminator.__init__

    def fwd(self, x):
        y = orig_fwd(self, x)
        if x.dim() == 2:
            c = x.coalesce()
            cap['tpl'].append(sha(c.indices()[0].numpy().astype(np.int32), c.indices()[1].numpy().astype(np.int32), c.values().numpy().astype(np.float32)))
        else:
            cap['final_Y'].append(y.detach().numpy().copy())
        return y

    def backward(self, *a, **k):
        cap['loss'].append(float(self.item()))
        return orig_backward(self, *a, **k)

    def step(self, *a, **k):
        r = orig_step(self, *a, **k)
        cap['n_steps'] = cap.get('n_steps', 0) + 1
        if cap['n_steps'] in CKPT:
            cap['ckpt'][cap['n_steps']] = {n: p.detach().numpy().copy() for n, p in cap['params'].items()}
        return r

    def d_init(self, size):
        orig_init(self, size)
        cap['D'] = self

    RA.Generator.forward, torch.Tensor.backward, torch.optim.Adam.step, RA.Discriminator.__init__ = fwd, backward, step, d_init
    orig_gen_init = RA.Generator.__init__

    def g_init(self, size, layer=2):
        orig_gen_init(self, size, layer)
        cap['G'] = self
    RA.Generator.__init__ = g_init
    orig_adam_init = torch.optim.Adam.__init__

    def adam_init(self, params, *a, **k):
        params = list(params)
        if cap.get('init') is None and 'D' in cap:
            cap['params'] = params_of(cap['G'], cap['D'])
            cap['init'] = {n: p.detach().numpy().copy() for n, p in cap['params'].items()}
        return orig_adam_init(self, params, *a, **k)
    torch.optim.Adam.__init__ = adam_init
    try:
        reseed()
        with contextlib.redirect_stdout(io.StringIO()):
            res = atk.posionDataAttack()
    finally:
        RA.Generator.forward, torch.Tensor.backward, torch.optim.Adam.step = orig_fwd, orig_backward, orig_step
        RA.Discriminator.__init__, RA.Generator.__init__, torch.optim.Adam.__init__ = orig_init, orig_gen_init, orig_adam_init
    return atk, res, cap


def sample_param(name, a):
    return a[[0, 7, a.shape[0] - 1]] if a.ndim == 2 and a.shape[0] > 1 else a


def main():
    out = {}
    shilling(out)
    atk, res, cap = aush(4)
    _, _, cap1 = aush(1)
    out['aush_targets'] = np.array(atk.targetItem, np.int32)
    out['aush_select'] = np.array(atk.selectItem, np.int32)
    for n in PARAMS:
        out['aush_init_sha__' + n] = np.array(sha(cap['init'][n].astype(np.float32)))
        out['aush_init_row__' + n] = cap['init'][n].reshape(cap['init'][n].shape[0], -1)[0].astype(np.float32)
    out['aush_tpl_sha'] = np.array(cap['tpl'])
    assert len(cap['loss']) == 2500 and len(cap['tpl']) == 2500, (len(cap['loss']), len(cap['tpl']))
    out['aush_loss'] = np.array(cap['loss'], np.float64)
    out['aush_loss_t1'] = np.array(cap1['loss'], np.float64)
    out['aush_ckpt_steps'] = np.array(CKPT, np.int64)
    for n in PARAMS:
        out['aush_ckpt__' + n] = np.stack([sample_param(n, cap['ckpt'][s][n]) for s in CKPT]).astype(np.float32)
        out['aush_ckpt_t1__' + n] = np.stack([sample_param(n, cap1['ckpt'][s][n]) for s in CKPT]).astype(np.float32)
    out['aush_final_Y'] = np.stack(cap['final_Y']).astype(np.float32)
    out['aush_row'], out['aush_col'], out['aush_val'] = block(res, atk.userNum)
    G.save('g30_shilling.npz', **out)


if __name__ == '__main__':
    main()

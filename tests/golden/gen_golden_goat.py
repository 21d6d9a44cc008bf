#!/usr/bin/env python3
"""Golden vectors for GOAT: runs the reference's own attack/Gray/GOAT.py on the CPU (ml-100k, seedSet(2018)) with the shims of gen_golden.py
and writes g32_goat.npz (data only).

The attack is built like g30's (maliciousUserSize = 0.01 -> 9 fake users, 5 unpopular targets) after seedSet(2018) and a fresh DataLoader;
`random.seed(SEED); np.random.seed(SEED); torch.manual_seed(SEED)` precede every captured call (SEED = 11, or the next seed whose long run
meets the two conditions below).

  g32_goat.npz
    seed                                 the seed used
    targets, item_int_num [1412]         internal target ids, itemIntNum
    samp<k>_Is / _If / _real             [4, 9, .] four consecutive itemSample calls at maliciousFeedbackSize 0 / 100 / 300 (k = 46 / 100 / 300)
    samp<k>_state_sha                    [4] SHA-256 of repr(random.getstate()) after every call
    init_sha__<p>                        digest of each initial parameter of the default attack (G.G_e.net.layer_0.weight, ... D.D_r.net.layer_3.bias)
    short run (BiLevelOptimizationEpoch = 2, epoch1 = 3, epoch2 = 2):
      short_loss1, short_loss2 (+ _t1)   [6] / [4] loss1 of every D step, loss2 of every G step, at four torch threads / at one
      short_z_sha                        [11] digest of every Z handed to G (the ten steps', then the final generation's)
      short_final__<p> (+ _t1)           the parameters at the end
      short_random_state_sha, short_numpy_state_sha, short_torch_state_sha
    long run (10 / 20 / 20):
      final_Y [9, 46], final_Is, final_If the last G outputs and the sample they belong to;  row / col / val: the fake block as COO in CSR order
      cut_margin [9]                     the n-th minus the (n + 1)-th largest value of each dense row before the projection (n = 46)
      targets_kept [9]                   how many of the 5 targets each fake row keeps
      long_random_state_sha, long_numpy_state_sha, long_torch_state_sha

Asserted before writing: in the long run every fake row keeps all targets and no value of final_Y is <= 0 -- then the projection is decided by
G's outputs alone (no tie among the targets' ones, no zero of the dense row above an output).

Usage:  python tests/golden/gen_golden_goat.py
"""
import contextlib
import io
import os
import random
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer)
import gen_golden_shilling as GS                       # noqa: E402  (fresh_data, sha, attack_args)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
import attack.Gray.GOAT as RG                          # noqa: E402

SIZES = (0, 100, 300)
SEEDS = range(11, 31)


def reseed(seed):
    random.seed(seed); np.random.seed(seed); torch.manual_seed(seed)


def state_shas():
    st = np.random.get_state()
    return dict(random_state_sha=GS.sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8)),
                numpy_state_sha=GS.sha(np.asarray(st[1], np.uint32), np.asarray([st[2]], np.int64)),
                torch_state_sha=GS.sha(torch.get_rng_state().numpy()))


def build(mfs=0):
    data = GS.fresh_data()
    a = GS.attack_args('GOAT', 'Gray')
    a.maliciousFeedbackSize = mfs
    with contextlib.redirect_stdout(io.StringIO()):
        return RG.GOAT(a, data)


def params_of(atk):
    return dict([('G.' + n, p) for n, p in atk.G.named_parameters()] + [('D.' + n, p) for n, p in atk.D.named_parameters()])


def samples(out):
    for mfs in SIZES:
        atk = build(mfs)
        k = atk.maliciousFeedbackNum
        reseed(11)
        Is, If, real, shas = [], [], [], []
        for call in range(4):
            I_s, I_f, rl = atk.itemSample(k, 0.01, 0.1, 0.02)
            Is.append(np.array(I_s, np.int32)); If.append(np.array(I_f, np.int32)); real.append(np.array(rl).astype(np.uint8))
            assert (np.array(rl) == real[-1]).all()
            shas.append(GS.sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8)))
        tag = 'samp%d_' % k
        out[tag + 'Is'], out[tag + 'If'], out[tag + 'real'], out[tag + 'state_sha'] = np.stack(Is), np.stack(If), np.stack(real), np.array(shas)


def run(threads, seed, be, e1, e2):
    torch.set_num_threads(threads)
    atk = build()
    atk.BiLevelOptimizationEpoch = be
    cap = dict(loss1=[], loss2=[], z=[], Y=[], init=None, sample=None)
    orig_fwd, orig_backward, orig_sample = RG.Encoder.forward, torch.Tensor.backward, atk.itemSample

    def fwd(self, x):
        y = orig_fwd(self, x)
        cap['z'].append(GS.sha(x.detach().numpy().astype(np.float32)))
        cap['Y'] = y.detach().numpy().copy()
        return y

    def backward(self, *a, **k):
        cap['loss1' if atk.D.training else 'loss2'].append(float(self.item()))
        return orig_backward(self, *a, **k)

    def sample(*a, **k):
        if cap['init'] is None:                                   # the first call precedes every step
            cap['init'] = {n: p.detach().numpy().copy() for n, p in params_of(atk).items()}
        cap['sample'] = orig_sample(*a, **k)
        return cap['sample']

    RG.Encoder.forward, torch.Tensor.backward, atk.itemSample = fwd, backward, sample
    try:
        reseed(seed)
        with contextlib.redirect_stdout(io.StringIO()):
            res = atk.posionDataAttack(epoch1=e1, epoch2=e2)
    finally:
        RG.Encoder.forward, torch.Tensor.backward = orig_fwd, orig_backward
    cap.update(state_shas())
    return atk, res, cap


def long_run(seed):
    atk, res, cap = run(4, seed, 10, 20, 20)
    I_s, I_f, _ = cap['sample']
    Y, n, tg = cap['Y'].astype(np.float32), atk.maliciousFeedbackNum, np.array(atk.targetItem)
    F = atk.fakeUserNum
    margin, kept = np.zeros(F, np.float64), np.zeros(F, np.int64)
    blk = res.tocsr()[atk.userNum:]
    for f in range(F):
        row = np.zeros(atk.itemNum, np.float32)
        row[np.array(I_s[f] + I_f[f])] = Y[f]
        row[tg] = 1
        v = np.sort(row)[::-1]
        margin[f] = float(v[n - 1]) - float(v[n])
        kept[f] = len(set(blk[f].indices.tolist()) & set(tg.tolist()))
    ok = bool((kept == len(tg)).all() and (Y > 0).all())
    return ok, atk, res, cap, Y, margin, kept


def main():
    warnings.simplefilter('ignore')
    out = {}
    atk = build()
    out['targets'], out['item_int_num'] = np.array(atk.targetItem, np.int32), np.array(atk.itemIntNum, np.float64)
    samples(out)
    for seed in SEEDS:
        ok, atk, res, cap, Y, margin, kept = long_run(seed)
        if ok:
            break
    assert ok, 'no seed whose long run keeps all targets with positive outputs'
    assert (kept == len(atk.targetItem)).all() and (Y > 0).all()
    out['seed'] = np.array(seed, np.int64)
    I_s, I_f, _ = cap['sample']
    out['final_Y'], out['final_Is'], out['final_If'] = Y, np.array(I_s, np.int32), np.array(I_f, np.int32)
    out['row'], out['col'], out['val'] = GS.block(res, atk.userNum)
    out['cut_margin'], out['targets_kept'] = margin, kept
    for key in ('random_state_sha', 'numpy_state_sha', 'torch_state_sha'):
        out['long_' + key] = np.array(cap[key])
    atk4, _, c4 = run(4, seed, 2, 3, 2)
    atk1, _, c1 = run(1, seed, 2, 3, 2)
    assert len(c4['loss1']) == 6 and len(c4['loss2']) == 4 and len(c4['z']) == 11, [len(c4[k]) for k in ('loss1', 'loss2', 'z')]
    assert c1['z'] == c4['z'] and c1['random_state_sha'] == c4['random_state_sha'] and c1['torch_state_sha'] == c4['torch_state_sha']
    for n, p in c4['init'].items():
        out['init_sha__' + n] = np.array(GS.sha(p.astype(np.float32)))
        assert (c1['init'][n] == p).all(), n
    out['short_loss1'], out['short_loss1_t1'] = np.array(c4['loss1'], np.float64), np.array(c1['loss1'], np.float64)
    out['short_loss2'], out['short_loss2_t1'] = np.array(c4['loss2'], np.float64), np.array(c1['loss2'], np.float64)
    out['short_z_sha'] = np.array(c4['z'])
    for n, p in params_of(atk4).items():
        out['short_final__' + n] = p.detach().numpy().astype(np.float32)
    for n, p in params_of(atk1).items():
        out['short_final_t1__' + n] = p.detach().numpy().astype(np.float32)
    for key in ('random_state_sha', 'numpy_state_sha', 'torch_state_sha'):
        out['short_' + key] = np.array(c4[key])
    G.save('g32_goat.npz', **out)
    print('seed', seed, '\nloss1', c4['loss1'], c1['loss1'], '\nloss2', c4['loss2'], c1['loss2'], '\ncut_margin', margin.tolist(), '\nkept', kept.tolist(),
          'Y min/max', Y.min(), Y.max())


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""Golden vectors for LegUP: runs the reference's own attack/Gray/LegUP.py on the CPU (ml-100k, seedSet(2018)) with the shims of gen_golden.py
and writes g31_legup.npz (data only).

The attack is built like g30's (maliciousUserSize = 0.01 -> 9 fake users, maliciousFeedbackSize = 0, 5 unpopular targets) after seedSet(2018)
and a fresh DataLoader; `random.seed(11); np.random.seed(11); torch.manual_seed(11)` precede the call.  It is shrunk through the reference's
own knobs only: BiLevelOptimizationEpoch = 2, Tepoch = 2, posionDataAttack(epoch1=3, epoch2=2), and `--maxEpoch 1` for the parser its own
LightGCN is built from (its other defaults stand: emb_size 64, n_layers 2, batch_size 2048): 6 D steps, 4 G steps, 8 one-epoch trainings.

  g31_legup.npz
    targets, select                      internal target ids, selectItem
    init_sha__<p>                        digest of each initial parameter (G.net.layer_0.weight, ... D.net.0.bias)
    tpl_sha                              [6 + 1] SHA-256 of every template handed to G (the D steps', then the final generation's rows)
    loss1, loss1_t1                      [6] loss1 of every D step at four torch threads / at one
    num_samples, edge_sha                [8] number and digest (int32 rows, cols sorted by row then column) of every sampled edge set
    loss2, loss2_t1                      [4] L_RS of every G step (the last of its Tepoch) at four threads / at one
    lrs_all, lrs_all_t1                  [8] L_RS of every inner iteration
    final_D__<p>, final_D_t1__<p>        D's parameters at the end
    final_G_sha__<p>                     digest of G's parameters at the end (equal to init_sha: L_RS does not reach G)
    final_Y                              [9, S] the final G outputs;  row / col / val: the fake block as COO in CSR order
    random_state_sha, numpy_state_sha    SHA-256 of repr(random.getstate()) / of numpy's MT state words and position afterwards
    near_threshold_share                 share of final_Y entries within 1e-4 of the 0.1 threshold (checked < 1e-3 here)

Usage:  python tests/golden/gen_golden_legup.py
"""
import contextlib
import io
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer)
import gen_golden_shilling as GS                       # noqa: E402  (fresh_data, reseed, block, sha, attack_args, PARAMS)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
import attack.Gray.LegUP as RL                         # noqa: E402
import recommender.LightGCN as RG                      # noqa: E402

PARAMS = GS.PARAMS
NEAR_EPS, NEAR_CAP = 1e-4, 1e-3


def edge_sha(rows, cols):
    o = np.lexsort((cols, rows))
    return GS.sha(rows[o].astype(np.int32), cols[o].astype(np.int32))


def numpy_state_sha():
    st = np.random.get_state()
    return GS.sha(np.asarray(st[1], np.uint32), np.asarray([st[2]], np.int64))


def legup(threads):
    torch.set_num_threads(threads)
    data = GS.fresh_data()
    argv, sys.argv = sys.argv, ['legup', '--dataset', 'ml-100k', '--data_path', G.REF + '/data/clean/', '--maxEpoch', '1']
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            atk = RL.LegUP(GS.attack_args('LegUP', 'Gray'), data)
    finally:
        sys.argv = argv
    atk.BiLevelOptimizationEpoch, atk.Tepoch = 2, 2
    cap = dict(tpl=[], loss1=[], loss2=[], lrs=[], samples=[], final_Y=[], init=None, training=False)
    orig = dict(fwd=RL.Generator.forward, backward=torch.Tensor.backward, g_init=RL.Generator.__init__, d_init=RL.Discriminator.__init__,
                adam_init=torch.optim.Adam.__init__, train=RG.LightGCN.train, init_adj=RG.LGCN_Encoder._init_uiAdj, tsum=torch.sum)

    def fwd(self, x):
        y = orig['fwd'](self, x)
        c = x.coalesce()
        if x.dim() == 2:
            cap['tpl'].append(GS.sha(c.indices()[0].numpy().astype(np.int32), c.indices()[1].numpy().astype(np.int32), c.values().numpy().astype(np.float32)))
        else:
            cap['final_Y'].append(y.detach().numpy().copy())
            cap.setdefault('final_rows', []).append((c.indices()[0].numpy().astype(np.int32), c.values().numpy().astype(np.float32)))
        return y

    def backward(self, *a, **k):
        if not cap['training']:
            cap['loss1' if cap['D'].training else 'loss2'].append(float(self.item()))
        return orig['backward'](self, *a, **k)

    def tsum(x, *a, **k):
        r = orig['tsum'](x, *a, **k)
        if not cap['training'] and not a and not k and isinstance(x, torch.Tensor) and x.dim() == 3:            # the [U, T, I] log-ratio tensor of L_RS
            cap['lrs'].append(-float(r))
        return r

    def train(self, *a, **k):
        cap['training'] = True
        try:
            return orig['train'](self, *a, **k)
        finally:
            cap['training'] = False

    def init_adj(self, ui_adj):
        U = self.data.user_num
        m = ui_adj.tocoo()
        up = m.row < U
        cap['samples'].append((int(up.sum()), edge_sha(m.row[up], m.col[up] - U)))
        return orig['init_adj'](self, ui_adj)

    def g_init(self, size, layer=2):
        orig['g_init'](self, size, layer)
        cap['G'] = self

    def d_init(self, size):
        orig['d_init'](self, size)
        cap['D'] = self

    def adam_init(self, params, *a, **k):
        params = list(params)
        if cap['init'] is None and 'D' in cap:
            cap['init'] = {n: p.detach().numpy().copy() for n, p in GS.params_of(cap['G'], cap['D']).items()}
        return orig['adam_init'](self, params, *a, **k)

    RL.Generator.forward, torch.Tensor.backward, RL.Generator.__init__, RL.Discriminator.__init__ = fwd, backward, g_init, d_init
    torch.optim.Adam.__init__, RG.LightGCN.train, RG.LGCN_Encoder._init_uiAdj, torch.sum = adam_init, train, init_adj, tsum
    try:
        GS.reseed()
        with contextlib.redirect_stdout(io.StringIO()):
            res = atk.posionDataAttack(epoch1=3, epoch2=2)
    finally:
        RL.Generator.forward, torch.Tensor.backward, RL.Generator.__init__, RL.Discriminator.__init__ = orig['fwd'], orig['backward'], orig['g_init'], orig['d_init']
        torch.optim.Adam.__init__, RG.LightGCN.train, RG.LGCN_Encoder._init_uiAdj, torch.sum = orig['adam_init'], orig['train'], orig['init_adj'], orig['tsum']
    cap['random_state_sha'] = GS.sha(np.frombuffer(repr(random.getstate()).encode(), np.uint8))
    cap['numpy_state_sha'] = numpy_state_sha()
    return atk, res, cap


def main():
    atk, res, cap = legup(4)
    _, _, cap1 = legup(1)
    assert len(cap['loss1']) == 6 and len(cap['loss2']) == 4 and len(cap['samples']) == 8 and len(cap['lrs']) == 8 and len(cap['tpl']) == 6, \
        [len(cap[k]) for k in ('loss1', 'loss2', 'samples', 'lrs', 'tpl')]
    assert cap1['samples'] == cap['samples'] and cap1['tpl'] == cap['tpl']
    assert np.allclose(cap['loss2'], cap['lrs'][1::2], rtol=1e-6)
    out = dict(targets=np.array(atk.targetItem, np.int32), select=np.array(atk.selectItem, np.int32))
    final = GS.params_of(atk.G, atk.D)
    final1 = GS.params_of(cap1['G'], cap1['D'])
    for n in PARAMS:
        out['init_sha__' + n] = np.array(GS.sha(cap['init'][n].astype(np.float32)))
        if n.startswith('G.'):
            out['final_G_sha__' + n] = np.array(GS.sha(final[n].detach().numpy().astype(np.float32)))
            assert str(out['final_G_sha__' + n]) == str(out['init_sha__' + n]), n          # quirk: G never moves
        else:
            out['final_D__' + n] = final[n].detach().numpy().astype(np.float32)
            out['final_D_t1__' + n] = final1[n].detach().numpy().astype(np.float32)
    fr = cap['final_rows']
    final_tpl = GS.sha(np.concatenate([np.full(len(c), i, np.int32) for i, (c, v) in enumerate(fr)]), np.concatenate([c for c, v in fr]),
                       np.concatenate([v for c, v in fr]))
    out['tpl_sha'] = np.array(cap['tpl'] + [final_tpl])
    out['loss1'], out['loss1_t1'] = np.array(cap['loss1'], np.float64), np.array(cap1['loss1'], np.float64)
    out['loss2'], out['loss2_t1'] = np.array(cap['loss2'], np.float64), np.array(cap1['loss2'], np.float64)
    out['lrs_all'], out['lrs_all_t1'] = np.array(cap['lrs'], np.float64), np.array(cap1['lrs'], np.float64)
    out['num_samples'] = np.array([n for n, _ in cap['samples']], np.int64)
    out['edge_sha'] = np.array([s for _, s in cap['samples']])
    Y = np.stack(cap['final_Y']).astype(np.float32)
    out['final_Y'] = Y
    share = float((np.abs(Y - 0.1) <= NEAR_EPS).mean())
    assert share < NEAR_CAP, share                          # the cap tests/test_gpu_legup.py asserts on the fixture
    out['near_threshold_share'] = np.array(share)
    out['row'], out['col'], out['val'] = GS.block(res, atk.userNum)
    out['random_state_sha'], out['numpy_state_sha'] = np.array(cap['random_state_sha']), np.array(cap['numpy_state_sha'])
    G.save('g31_legup.npz', **out)
    print('loss1', cap['loss1'], '\nloss2', cap['loss2'], cap1['loss2'], '\nnum_samples', out['num_samples'].tolist(), 'near share', share)


if __name__ == '__main__':
    main()

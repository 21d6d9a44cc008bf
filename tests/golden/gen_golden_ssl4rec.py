#!/usr/bin/env python3
"""Golden vectors for SSL4Rec: runs the reference's own recommender/SSL4Rec.py on CPU (ml-100k, emb 64) with the shims of gen_golden.py and the
writer helpers of gen_golden_models.py, and writes g29_ssl4rec.npz (data only, large arrays as SAMPLE_ROWS sampled rows).

The reference's `model.dropout` (nn.Dropout(0.2), SSL4Rec.py:187, called four times per step by item_encoding :232-241: user view 1, user
view 2, item view 1, item view 2) is replaced during every run by a deterministic mask source:

    the c-th call (c = 0..3) of step t keeps element (i, k) iff  numpy.random.default_rng([2018, t, c]).random((n, d))[i, k] >= 0.2
    and returns x * keep * 1.25;  t counts the steps of one run from 0 (across epochs), n = the batch size, d = 64.

The product's tests rebuild the same masks from this rule (tests/test_ssl4rec_cpu.py, tests/test_gpu_ssl4rec.py), so no mask is stored;
`mask_sha` is a SHA-256 over the boolean masks of the 25-step run, in call order.

  g29_ssl4rec.npz
    param_names, init_sha__<param>, init_probe__<param>   parameter order, digest and first row of every initial parameter
    fwd_user / fwd_item                                   the initial full-table forward
    grad0__embedding_dict.<table>                         step-0 gradients of both tables
    rec_losses, cl_losses, batch_sizes, batches_sha       25 Adam steps (Adam over model.parameters(), towers included)
    final__embedding_dict.<table>, tower_sha__<param>     the tables after 25 steps, and digests of the towers (equal to init_sha: never moved)
    mask_sha                                              digest of the 25 steps' masks
    api_*                                                 SSL4Rec(args, data).train(Epoch=2, evalNum=1, requires_embgrad=True)
    adj_block                                             SSL4Rec(args, data).train(Epoch=1, evalNum=1, requires_adjgrad=True) (Matgrad block)

Usage:  python tests/golden/gen_golden_ssl4rec.py
"""
import contextlib
import copy
import hashlib
import io
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer)
import gen_golden_models as GM                         # noqa: E402  (row sampling and digests)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
from util.tool import seedSet                          # noqa: E402
from util.DataLoader import DataLoader                 # noqa: E402
from util import sampler as ref_sampler                # noqa: E402
from util import loss as ref_loss                      # noqa: E402
from recommender.SSL4Rec import SSL4Rec                # noqa: E402

STEPS = 25
DROP = 0.2
MASK_SEED = 2018


def rule_mask(t, c, n, d):
    """The deterministic dropout mask of call c (0: user view 1, 1: user view 2, 2: item view 1, 3: item view 2) of step t."""
    return np.random.default_rng([MASK_SEED, t, c]).random((n, d)) >= DROP


class RuleDropout(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.calls = 0
        self.masks = []

    def forward(self, x):
        t, c = divmod(self.calls, 4)
        self.calls += 1
        m = rule_mask(t, c, x.shape[0], x.shape[1])
        self.masks.append(m)
        return x * torch.from_numpy(m.astype(np.float32)) * (1.0 / (1.0 - DROP))


def fresh(args):
    seedSet(2018)
    data = DataLoader(args)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = SSL4Rec(args, data)
    rec.model.dropout = RuleDropout()
    return data, rec


def main():
    args = G.rec_args(emb_size=64, model_name='SSL4Rec')
    seedSet(2018)
    data = DataLoader(args)
    training0 = [list(r) for r in data.training_data]
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = SSL4Rec(args, data)
    model = rec.model
    model.dropout = RuleDropout()
    o = {'param_names': np.array([n for n, _ in model.named_parameters()])}
    for n, v in GM.params(model).items():
        o['init_sha__' + n], o['init_probe__' + n] = GM.sha(v), v.reshape(v.shape[0], -1)[0].copy()
    with torch.no_grad():
        u, i = model()
    GM.put(o, 'fwd_user', u.numpy()); GM.put(o, 'fwd_item', i.numpy())

    # 25 steps of the reference loop body (SSL4Rec.py:55-75) with the default Adam(model.parameters())
    optim = torch.optim.Adam(model.parameters(), lr=args.lRate)
    random.seed(2018)
    d2 = copy.copy(data)
    d2.training_data = [list(r) for r in training0]
    rec_losses, cl_losses, batches = [], [], []
    step = 0
    while step < STEPS:
        for user_idx, pos_idx, neg_idx in ref_sampler.next_batch_pairwise(d2, args.batch_size):
            model.train()
            rec_user_emb, rec_item_emb = model()
            user_emb, pos_item_emb, neg_item_emb = rec_user_emb[user_idx], rec_item_emb[pos_idx], rec_item_emb[neg_idx]
            rec_loss = ref_loss.bpr_loss(user_emb, pos_item_emb, neg_item_emb)
            cl_loss = rec.cl_rate * model.cal_cl_loss(user_idx, pos_idx)
            batch_loss = rec_loss + ref_loss.l2_reg_loss(args.reg, user_emb, pos_item_emb) + cl_loss
            optim.zero_grad()
            batch_loss.backward()
            if step == 0:
                for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
                    GM.put(o, 'grad0__' + n, dict(model.named_parameters())[n].grad.numpy())
            optim.step()
            rec_losses.append(rec_loss.item()); cl_losses.append(cl_loss.item())
            batches.append((user_idx, pos_idx, neg_idx))
            step += 1
            if step >= STEPS:
                break
    for n, v in GM.params(model).items():
        if n.startswith('embedding_dict.'):
            GM.put(o, 'final__' + n, v)
        else:
            o['tower_sha__' + n] = GM.sha(v)
    o['rec_losses'] = np.array(rec_losses, np.float32)
    o['cl_losses'] = np.array(cl_losses, np.float32)
    o['batch_sizes'] = np.array([len(b[0]) for b in batches], np.int64)
    o['batches_sha'] = GM.batches_sha(batches)
    h = hashlib.sha256()
    for m in model.dropout.masks:
        h.update(np.ascontiguousarray(m, dtype=np.bool_).tobytes())
    o['mask_sha'] = np.array(h.hexdigest())

    # the class surface end to end
    data, rec = fresh(args)
    with contextlib.redirect_stdout(io.StringIO()):
        ue, ie, ug, ig = rec.train(Epoch=2, evalNum=1, requires_embgrad=True)
        _, measure = rec.test()
    GM.put(o, 'api_user_emb', ue.detach().numpy()); GM.put(o, 'api_item_emb', ie.detach().numpy())
    GM.put(o, 'api_usergrad', ug.detach().numpy()); GM.put(o, 'api_itemgrad', ig.detach().numpy())
    o['api_best_epoch'] = np.array([rec.bestPerformance[0]], np.int64)
    o['api_measure'] = np.array([float(m.strip().split(':')[1]) for m in measure[1:]], np.float64)
    o['api_next_random'] = np.array([random.random()], np.float64)

    data, rec = fresh(args)
    with contextlib.redirect_stdout(io.StringIO()):
        block = rec.train(Epoch=1, evalNum=1, requires_adjgrad=True)
    GM.put(o, 'adj_block', block.detach().numpy())
    G.save('g29_ssl4rec.npz', **o)


if __name__ == '__main__':
    torch.set_num_threads(4)
    main()

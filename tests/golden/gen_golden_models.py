#!/usr/bin/env python3
"""Golden vectors for NCF and WRMF: runs the reference's own recommender/NCF.py and recommender/WRMF.py on CPU (ml-100k, emb 64) with the
shims of gen_golden.py (numba stub, .cuda() = identity) and writes data only, kept small:

  * a 2-D array of more than SAMPLE_ROWS rows is stored as SAMPLE_ROWS of its rows, `<key>` = those rows and `<key>__rows` = their indices
    (a fixed random choice per row count); smaller arrays and vectors are stored whole;
  * what a test rebuilds exactly is stored as a SHA-256 of its bytes: the initial parameters (the product draws the same ones under
    seedSet(2018)) and the 25 training batches (the product's drop-in sampler after random.seed(2018) on a fresh DataLoader).

  g27_ncf.npz / g28_wrmf.npz
    param_names, init_sha__<param>   parameter order (model.named_parameters()) and a digest of every initial parameter (float32 bytes)
    init_probe__<param>              its first row (a readable spot check next to the digest)
    fwd_user / fwd_item              the full-table forward of the initial model
    grad0__<param>                   step-0 gradient of every parameter (the reference loop body, bpr / wrmf loss + l2)
    losses, batch_sizes, batches_sha 25 Adam steps (more than one 22-batch epoch)
    final__<param>                   the tables after the 25 steps (NCF: the MF tables; WRMF: both);  m_state / v_state: Adam state of
                                     adam_state_param (WRMF only: NCF's tower trajectory is not reproducible, see tests/test_gpu_ncf.py)
    api_*                            X(args, data).train(Epoch=2, evalNum=1, requires_embgrad=True): returned tensors, measure lines, best epoch,
                                     next value of python `random`

Usage:  python tests/golden/gen_golden_models.py            (writes tests/golden/g27_ncf.npz and g28_wrmf.npz)
"""
import copy
import contextlib
import hashlib
import io
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer; its __main__ does not run)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
from util.tool import seedSet                          # noqa: E402
from util.DataLoader import DataLoader                 # noqa: E402
from util import sampler as ref_sampler                # noqa: E402
from util import loss as ref_loss                      # noqa: E402
from recommender.NCF import NCF                        # noqa: E402
from recommender.WRMF import WRMF                      # noqa: E402

STEPS = 25
SAMPLE_ROWS = 32
ADAM_STATE = {'wrmf': 'embedding_dict.item_emb'}


def sample_rows(n):
    return np.sort(np.random.default_rng(n).choice(n, SAMPLE_ROWS, replace=False)).astype(np.int32)


def put(o, key, arr):
    arr = np.asarray(arr)
    if arr.ndim == 2 and arr.shape[0] > SAMPLE_ROWS:
        r = sample_rows(arr.shape[0])
        o[key], o[key + '__rows'] = arr[r].copy(), r
    else:
        o[key] = arr.copy()


def sha(arr):
    return np.array(hashlib.sha256(np.ascontiguousarray(arr, dtype=np.float32).tobytes()).hexdigest())


def batches_sha(batches):
    h = hashlib.sha256()
    for u, p, n in batches:
        for x in (u, p, n):
            h.update(np.asarray(x, dtype=np.int32).tobytes())
    return np.array(h.hexdigest())


def params(model):
    return {n: p.detach().numpy().copy() for n, p in model.named_parameters()}


def run(name, cls, loss_fn):
    args = G.rec_args(emb_size=64, model_name=cls.__name__)
    seedSet(2018)
    data = DataLoader(args)
    training0 = [list(r) for r in data.training_data]
    seedSet(2018)
    rec = cls(args, data)
    model = rec.model
    o = {'param_names': np.array([n for n, _ in model.named_parameters()])}
    for n, v in params(model).items():
        o['init_sha__' + n], o['init_probe__' + n] = sha(v), v.reshape(v.shape[0], -1)[0].copy()
    with torch.no_grad():
        u, i = model()
    put(o, 'fwd_user', u.detach().numpy()); put(o, 'fwd_item', i.detach().numpy())
    optim = torch.optim.Adam(model.parameters(), lr=args.lRate)
    random.seed(2018)
    d2 = copy.copy(data)
    d2.training_data = [list(r) for r in training0]
    losses, batches = [], []
    step = 0
    while step < STEPS:
        for user_idx, pos_idx, neg_idx in ref_sampler.next_batch_pairwise(d2, args.batch_size):
            rec_user_emb, rec_item_emb = model()
            user_emb, pos_item_emb, neg_item_emb = rec_user_emb[user_idx], rec_item_emb[pos_idx], rec_item_emb[neg_idx]
            batch_loss = loss_fn(user_emb, pos_item_emb, neg_item_emb) + ref_loss.l2_reg_loss(args.reg, user_emb, pos_item_emb)
            optim.zero_grad()
            batch_loss.backward()
            if step == 0:
                for n, p in model.named_parameters():
                    put(o, 'grad0__' + n, p.grad.numpy())
            optim.step()
            losses.append(batch_loss.item())
            batches.append((user_idx, pos_idx, neg_idx))
            step += 1
            if step >= STEPS:
                break
    for n, v in params(model).items():
        if n.startswith('embedding_dict.') and (name == 'wrmf' or '_mf_' in n):
            put(o, 'final__' + n, v)
    if name in ADAM_STATE:
        st = optim.state[dict(model.named_parameters())[ADAM_STATE[name]]]
        put(o, 'm_state', st['exp_avg'].numpy()); put(o, 'v_state', st['exp_avg_sq'].numpy())
        o['adam_state_param'] = np.array(ADAM_STATE[name])
    o['losses'] = np.array(losses, np.float32)
    o['batch_sizes'] = np.array([len(b[0]) for b in batches], np.int64)
    o['batches_sha'] = batches_sha(batches)

    # the class surface end to end
    seedSet(2018)
    data = DataLoader(args)
    rec = cls(args, data)
    with contextlib.redirect_stdout(io.StringIO()):
        ue, ie, ug, ig = rec.train(Epoch=2, evalNum=1, requires_embgrad=True)
        _, measure = rec.test()
    put(o, 'api_user_emb', ue.detach().numpy()); put(o, 'api_item_emb', ie.detach().numpy())
    put(o, 'api_usergrad', ug.detach().numpy()); put(o, 'api_itemgrad', ig.detach().numpy())
    o['api_best_epoch'] = np.array([rec.bestPerformance[0]], np.int64)
    o['api_measure'] = np.array([float(m.strip().split(':')[1]) for m in measure[1:]], np.float64)
    o['api_next_random'] = np.array([random.random()], np.float64)
    G.save('g27_ncf.npz' if name == 'ncf' else 'g28_wrmf.npz', **o)


if __name__ == '__main__':
    torch.set_num_threads(4)
    run('ncf', NCF, ref_loss.bpr_loss)
    run('wrmf', WRMF, ref_loss.wrmf_loss)

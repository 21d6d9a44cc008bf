#!/usr/bin/env python3
"""Golden vectors for the rest of util.loss and for DirectAU: runs the reference's own util/loss.py (alignment_loss, uniformity_loss,
batch_softmax_loss, kl_divergence, js_divergence) and a DirectAU loop assembled from the reference's LGCN_Encoder, next_batch_pairwise and loss
functions on CPU, with the shims of gen_golden.py and the writer helpers of gen_golden_models.py.  Data only; the reference is imported, not copied.

  g33_pairloss.npz   (every array numeric; sets are named  <fn>_<kind>_<n>x<d>)
    unif_sets / unif_shapes              names and (n, d) of the uniformity input sets, in order; kinds:
        gauss : Gaussian rows of scale 0.05, stored as float16 (the float32 input is that array widened: exact)
        clust : four centres (float32 [4, d], row r belongs to centre r % 4) plus a 1e-3 jitter stored as float16, x = centre + jitter in float32;
                then row 1 := row 0 (an exact copy) and, where it exists, row 3 := 0.  Stored as <set>__centres and <set>__jitter
    <set>__x                             gauss: the input (float16)
    <set>__loss32 / __loss64             the reference function's value on the float32 / the .double() input
    <set>__grad32 / __grad64             its input gradient (sampled rows beyond 32 rows: <key>__rows, as gen_golden_models.put)
    <set>__loss_err                      |loss32 - loss64|
    <set>__grad_err                      ||grad32 - grad64||_F / ||grad64||_F  (0 where grad64 is identically 0)
    <set>__grad_rowerr                   the same per row [n]
    align_130x64__x / __y                alignment inputs (row 5 of y is a positive multiple of row 5 of x: an identical normalised pair)
    align_130x64__same_row               the index of that pair
    align_130x64_a<alpha>__*             loss32, loss64, gradx64, grady64 (sampled rows), loss_err, gradx_err, grady_err (float32 against float64, as
                                         above), same_row_grads [4, d] (the pair's rows of the float32 and float64 gradients: zero) for alpha in {1, 2}
    bsm__* / kl__* / js__*               batch_softmax_loss (temperature 0.2), kl_divergence, js_divergence on one small input each:
                                         a, b, loss32, loss64, grada64, gradb64

  g34_directau.npz   ml-100k, d 64, L 2, seed 2018, gamma 2
    param_names, init_sha__*, init_probe__*, fwd_user / fwd_item, grad0__embedding_dict.<table>
    align_losses, unif_losses (gamma * (unif(u) + unif(p)) / 2), batch_sizes, batches_sha      25 Adam steps
    final__embedding_dict.<table>
    api_*      DirectAU(args, data).train(Epoch=2, evalNum=1, requires_embgrad=True) of a class made here from the reference's LightGCN: its own
               train loop with the two loss names of its module rebound to DirectAU's terms

Usage:  python tests/golden/gen_golden_pairloss.py [n_two_splits]
        n_two_splits: the smallest n with arl_uniformity_splits(n) >= 2 (default: asked from the built library)
"""
import contextlib
import copy
import io
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as G                                 # noqa: E402  (shims, argument builder, writer)
import gen_golden_models as GM                         # noqa: E402  (row sampling and digests)

import numpy as np                                     # noqa: E402
import torch                                           # noqa: E402
from util.tool import seedSet                          # noqa: E402
from util.DataLoader import DataLoader                 # noqa: E402
from util import sampler as ref_sampler                # noqa: E402
from util import loss as ref_loss                      # noqa: E402
import recommender.LightGCN as ref_lightgcn            # noqa: E402

STEPS = 25
GAMMA = 2.0
UNIF_SHAPES = [(2, 16), (17, 16), (130, 64), (1061, 128)]
TWO_SPLIT_WIDTH = 32


def two_split_rows():
    if len(sys.argv) > 1:
        return int(sys.argv[1])
    sys.path.insert(0, ROOT)
    from arlib_amd import _lib
    L = _lib.lib()
    n = 2
    while L.arl_uniformity_splits(n) < 2:
        n += 1
    return n


def gauss_rows(n, d):
    x16 = (np.random.default_rng([33, n, d]).standard_normal((n, d)) * 0.05).astype(np.float16)
    return {'x': x16}, x16.astype(np.float32)


def clust_rows(n, d):
    rng = np.random.default_rng([34, n, d])
    centres = rng.standard_normal((4, d)).astype(np.float32)
    jitter = (rng.standard_normal((n, d)) * 1e-3).astype(np.float16)
    return {'centres': centres, 'jitter': jitter}, clust_input(centres, jitter)


def clust_input(centres, jitter):
    x = centres[np.arange(jitter.shape[0]) % 4] + jitter.astype(np.float32)
    x[1] = x[0]
    if x.shape[0] > 3:
        x[3] = 0.0
    return x


def value_and_grads(fn, arrays, dtype):
    ts = [torch.from_numpy(a).to(dtype).requires_grad_(True) for a in arrays]
    loss = fn(*ts)
    grads = torch.autograd.grad(loss, ts)
    return loss.item(), [g.numpy() for g in grads]


def norm_err(a32, a64):
    den = np.linalg.norm(a64)
    return np.array(np.linalg.norm(a32.astype(np.float64) - a64) / den if den > 0 else 0.0)


def row_err(a32, a64):
    num, den = np.linalg.norm(a32.astype(np.float64) - a64, axis=1), np.linalg.norm(a64, axis=1)
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)


def gen_pairloss():
    o = {}
    shapes = UNIF_SHAPES + [(two_split_rows(), TWO_SPLIT_WIDTH)]
    names = []
    for kind, make in (('gauss', gauss_rows), ('clust', clust_rows)):
        for n, d in shapes:
            name = 'unif_%s_%dx%d' % (kind, n, d)
            names.append(name)
            stored, x = make(n, d)
            for k, v in stored.items():
                o[name + '__' + k] = v
            l32, (g32,) = value_and_grads(ref_loss.uniformity_loss, [x], torch.float32)
            l64, (g64,) = value_and_grads(ref_loss.uniformity_loss, [x], torch.float64)
            o[name + '__loss32'], o[name + '__loss64'] = np.array(l32, np.float32), np.array(l64, np.float64)
            GM.put(o, name + '__grad32', g32); GM.put(o, name + '__grad64', g64)
            o[name + '__loss_err'] = np.array(abs(l32 - l64))
            o[name + '__grad_err'], o[name + '__grad_rowerr'] = norm_err(g32, g64), row_err(g32, g64)
            print('%-22s loss %.9f  |loss32 - loss64| %.2e  grad err %.2e  worst row %.2e' % (name, l64, abs(l32 - l64), o[name + '__grad_err'], o[name + '__grad_rowerr'].max()))
    o['unif_sets'] = np.array(names)
    o['unif_shapes'] = np.array(shapes * 2, np.int64)

    rng = np.random.default_rng(35)
    x, y = rng.standard_normal((130, 64)).astype(np.float32), rng.standard_normal((130, 64)).astype(np.float32)
    y[5] = 2.0 * x[5]                                      # exact in float32: the normalised rows are bit-identical
    o['align_130x64__x'], o['align_130x64__y'], o['align_130x64__same_row'] = x, y, np.array(5, np.int64)
    for alpha in (1, 2):
        fn = lambda a, b: ref_loss.alignment_loss(a, b, alpha)
        l32, (gx32, gy32) = value_and_grads(fn, [x, y], torch.float32)
        l64, (gx64, gy64) = value_and_grads(fn, [x, y], torch.float64)
        k = 'align_130x64_a%d__' % alpha
        o[k + 'loss32'], o[k + 'loss64'], o[k + 'loss_err'] = np.array(l32, np.float32), np.array(l64, np.float64), np.array(abs(l32 - l64))
        GM.put(o, k + 'gradx64', gx64); GM.put(o, k + 'grady64', gy64)
        o[k + 'same_row_grads'] = np.stack([gx32[5], gy32[5], gx64[5].astype(np.float32), gy64[5].astype(np.float32)])      # all zero: the identical pair
        o[k + 'gradx_err'], o[k + 'grady_err'] = norm_err(gx32, gx64), norm_err(gy32, gy64)
        print('%-22s loss %.9f  |loss32 - loss64| %.2e  grad err %.2e %.2e' % (k, l64, abs(l32 - l64), o[k + 'gradx_err'], o[k + 'grady_err']))

    a, b = rng.standard_normal((24, 16)).astype(np.float32), rng.standard_normal((24, 16)).astype(np.float32)
    for key, fn in (('bsm', lambda p, q: ref_loss.batch_softmax_loss(p, q, 0.2)), ('kl', ref_loss.kl_divergence), ('js', ref_loss.js_divergence)):
        l32, _ = value_and_grads(fn, [a, b], torch.float32)
        l64, (ga, gb) = value_and_grads(fn, [a, b], torch.float64)
        o[key + '__a'], o[key + '__b'] = a, b
        o[key + '__loss32'], o[key + '__loss64'], o[key + '__grada64'], o[key + '__gradb64'] = np.array(l32, np.float32), np.array(l64, np.float64), ga, gb
    G.save('g33_pairloss.npz', **o)


def directau_terms(user_emb, pos_item_emb):
    align = ref_loss.alignment_loss(user_emb, pos_item_emb)
    unif = GAMMA * (ref_loss.uniformity_loss(user_emb) + ref_loss.uniformity_loss(pos_item_emb)) / 2
    return align, unif


class DirectAU(ref_lightgcn.LightGCN):
    """The reference's LightGCN class and train loop; while it trains, the two loss names its module calls are DirectAU's terms."""

    def train(self, *a, **k):
        scale = 1.0 / self.args.batch_size
        saved = ref_lightgcn.bpr_loss, ref_lightgcn.l2_reg_loss
        ref_lightgcn.bpr_loss = lambda u, p, n: sum(directau_terms(u, p))
        ref_lightgcn.l2_reg_loss = lambda reg, *embs: saved[1](reg * scale, *embs)
        try:
            return super().train(*a, **k)
        finally:
            ref_lightgcn.bpr_loss, ref_lightgcn.l2_reg_loss = saved


def gen_directau():
    args = G.rec_args(emb_size=64, n_layers=2, model_name='DirectAU')
    seedSet(2018)
    data = DataLoader(args)
    training0 = [list(r) for r in data.training_data]
    seedSet(2018)
    model = ref_lightgcn.LGCN_Encoder(data, args.emb_size, args.n_layers)
    o = {'param_names': np.array([n for n, _ in model.named_parameters()])}
    for n, v in GM.params(model).items():
        o['init_sha__' + n], o['init_probe__' + n] = GM.sha(v), v.reshape(v.shape[0], -1)[0].copy()
    with torch.no_grad():
        u, i = model()
    GM.put(o, 'fwd_user', u.numpy()); GM.put(o, 'fwd_item', i.numpy())

    optim = torch.optim.Adam(model.parameters(), lr=args.lRate)
    random.seed(2018)
    d2 = copy.copy(data)
    d2.training_data = [list(r) for r in training0]
    align_losses, unif_losses, batches = [], [], []
    while len(batches) < STEPS:
        for user_idx, pos_idx, neg_idx in ref_sampler.next_batch_pairwise(d2, args.batch_size):
            model.train()
            rec_user_emb, rec_item_emb = model()
            user_emb, pos_item_emb = rec_user_emb[user_idx], rec_item_emb[pos_idx]
            align, unif = directau_terms(user_emb, pos_item_emb)
            batch_loss = align + unif + ref_loss.l2_reg_loss(args.reg / args.batch_size, user_emb, pos_item_emb)
            optim.zero_grad()
            batch_loss.backward()
            if not batches:
                for n in ('embedding_dict.user_emb', 'embedding_dict.item_emb'):
                    GM.put(o, 'grad0__' + n, dict(model.named_parameters())[n].grad.numpy())
            optim.step()
            align_losses.append(align.item()); unif_losses.append(unif.item())
            batches.append((user_idx, pos_idx, neg_idx))
            if len(batches) >= STEPS:
                break
    for n, v in GM.params(model).items():
        GM.put(o, 'final__' + n, v)
    o['align_losses'], o['unif_losses'] = np.array(align_losses, np.float32), np.array(unif_losses, np.float32)
    o['batch_sizes'] = np.array([len(b[0]) for b in batches], np.int64)
    o['batches_sha'] = GM.batches_sha(batches)

    seedSet(2018)
    data = DataLoader(args)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = DirectAU(args, data)
        ue, ie, ug, ig = rec.train(Epoch=2, evalNum=1, requires_embgrad=True)
        _, measure = rec.test()
    GM.put(o, 'api_user_emb', ue.detach().numpy()); GM.put(o, 'api_item_emb', ie.detach().numpy())
    GM.put(o, 'api_usergrad', ug.detach().numpy()); GM.put(o, 'api_itemgrad', ig.detach().numpy())
    o['api_best_epoch'] = np.array([rec.bestPerformance[0]], np.int64)
    o['api_measure'] = np.array([float(m.strip().split(':')[1]) for m in measure[1:]], np.float64)
    o['api_next_random'] = np.array([random.random()], np.float64)
    G.save('g34_directau.npz', **o)


if __name__ == '__main__':
    torch.set_num_threads(4)
    gen_pairloss()
    gen_directau()

#!/usr/bin/env python3
"""The exact item-kNN scoring op (arlib_amd/itemknn.py, csrc/arl_itemknn.hip) at ml-1M's shape (6 040 x 3 706, SYN-v1 pairs at ml-1M's mean degree)
and at cfg2's (SYN-v1, 1 M users x 100 K items), and the ItemKNN victim beside GMF under Random and Bandwagon poisoning on ml-100k.  Prints one
JSON line per part and writes profiles/itemknn_bench.json.

    python tools/itemknn_bench.py [--reps 5] [--k 50] [--n 50] [--subset 32768] [--full-limit-s 60] [--host-rows 256] [--skip-cfg2] [--skip-victims]

Per shape (the lists are neighbours.cooccur_topk on the transposed matrix, cosine weights; every profile is masked, N = --n):
  lists_ms       cooccur_topk(route='kernel') on the item side plus knn_weights, host clock, one run;
  plan_ms        the wrapper's preparation on the device (canonical rows, live-slot weights, launch order; host clock around a synchronise);
  kernel_ms      arl_itemknn_score_topk_i64 alone on that plan (device events; median, min, max of --reps after one warm-up), without targets
                 and with five; entries = the neighbour entries the kernel reads (live slots of the profile's items, times the tiles);
  host_s         itemknn.knn_score_topk_host on --host-rows of the queries, host clock, one run; and that the integers are equal;
  composed_ms    torch.sparse.mm of the fp32 weight matrix into dense chunks of --chunk query rows, the profile's items set to -inf, torch.topk.
                 A timing yardstick only: its fp32 sums and its order among ties are not the contract's; the share of rows whose list equals
                 the kernel's is reported.
At cfg2 the kernel is timed on --subset random queries (a test-sized query set) first, and on all users only when that predicts at most
--full-limit-s seconds; the composed route is timed on the same subset.

The victims: ml-100k (tests/golden/ml100k_data.npz), Random and Bandwagon at the reference's default budget (1 % fake users, five unpopular
targets), a GMF and an ItemKNN victim trained on the clean data, on the poisoned data and on the data after detect.sanitize dropped the F users
with the largest degsim, each read with TargetRankMetric (HitRate@50, ER@50, mean rank of the targets, training items masked).  A measurement to
report as it comes out, not a test and not a claim."""
import argparse
import contextlib
import io
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                            # noqa: E402
import scipy.sparse as sp                     # noqa: E402
from cooccur_bench import graph, events_ms, host_ms   # noqa: E402
from detect_bench import clean_data, loader_of        # noqa: E402


def shape(X, a, name):
    import torch
    from arlib_amd import _lib, itemknn, neighbours, ops
    U, I = X.shape
    k, N = a.k, a.n
    out = dict(shape=name, users=U, items=I, nnz=int(X.nnz), k=k, N=N, tile_items=itemknn.KNN_DEFAULT_TILE_ITEMS,
               tiles=-(-I // itemknn.KNN_DEFAULT_TILE_ITEMS), max_profile=int(np.diff(X.indptr).max()))
    XT = sp.csr_matrix(X.T)
    XT.sort_indices()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, cnt, deg = neighbours.cooccur_topk(XT.indptr.astype(np.int64), XT.indices.astype(np.int32), I, U, k, 'cosine', route='kernel')
    nbr_w = itemknn.knn_weights(idx, cnt, deg, 'cosine')
    out['lists_ms'] = (time.perf_counter() - t0) * 1e3
    ni, nw = idx.contiguous(), torch.from_numpy(nbr_w).cuda()
    rp, ci = torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda()

    def plan():
        crp, cci, r, _ = neighbours._canonical(rp, ci, U, I)
        weight = torch.zeros(U, dtype=torch.int64, device='cuda').index_add_(0, r, (ni >= 0).sum(1)[cci.long()])
        return crp, cci, weight
    out['plan_ms'] = host_ms(plan, a.reps)
    crp, cci, weight = plan()
    L, P = _lib.lib(), ops._ptr
    tg = torch.sort(torch.from_numpy(np.random.RandomState(2).choice(I, 5, replace=False).astype(np.int32))).values.cuda()
    tcol = torch.arange(5, dtype=torch.int32, device='cuda')

    def kernel(rows, T):
        Q = U if rows is None else rows.numel()
        wq = weight if rows is None else weight[rows.long()]
        order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
        oi, os_ = torch.empty((Q, N), dtype=torch.int32, device='cuda'), torch.empty((Q, N), dtype=torch.int64, device='cuda')
        rk = torch.empty((Q, max(T, 1)), dtype=torch.int32, device='cuda')
        run = lambda: _lib.check(L.arl_itemknn_score_topk_i64(P(crp), P(cci), U, I, P(ni), P(nw), k, P(rows), Q, N, 1, P(tg) if T else None,
                                                              P(tcol) if T else None, T, P(order), 0, P(oi), P(os_), P(rk) if T else None,
                                                              ops._stream()), 'arl_itemknn_score_topk_i64')
        return run, oi, os_, float(wq.sum()) * out['tiles']
    rng = np.random.RandomState(1)
    sub = None
    if U > a.subset:
        sub = torch.from_numpy(np.sort(rng.choice(U, a.subset, replace=False)).astype(np.int32)).cuda()
        run, oi, os_, ent = kernel(sub, 0)
        t = events_ms(run, max(2, a.reps // 2))
        out.update(subset_queries=a.subset, subset_kernel_ms=t, subset_entries=ent, subset_gentries_per_s=ent / t[0] / 1e6,
                   subset_kernel_5_targets_ms=events_ms(kernel(sub, 5)[0], max(2, a.reps // 2)), full_kernel_ms_predicted_from_subset=t[0] * U / a.subset)
        if t[0] * U / a.subset > a.full_limit_s * 1e3:
            out['kernel_ms'] = None
            out['note'] = 'all users not timed: the subset predicts more than --full-limit-s = %g s' % a.full_limit_s
    if 'kernel_ms' not in out:
        run, oi_all, os_all, ent = kernel(None, 0)
        t = events_ms(run, a.reps if sub is None else 2)
        out.update(kernel_ms=t, entries=ent, gentries_per_s=ent / t[0] / 1e6, kernel_ms_per_query=t[0] / U)
        if sub is None:
            out['kernel_5_targets_ms'] = events_ms(kernel(None, 5)[0], a.reps)
            out['call_ms'] = events_ms(lambda: itemknn.knn_score_topk(rp, ci, U, I, ni, nw, N, mask_profile=True, route='kernel'), a.reps)
            oi, os_ = oi_all, os_all
        else:
            del oi_all, os_all
    q_ids = np.arange(U) if sub is None else sub.cpu().numpy().astype(np.int64)
    # the host route on --host-rows of the timed queries
    pick = np.sort(rng.choice(len(q_ids), min(a.host_rows, len(q_ids)), replace=False))
    t0 = time.perf_counter()
    hi, hs, _ = itemknn.knn_score_topk_host(X, idx.cpu().numpy(), nbr_w, N, q_ids[pick], True)
    out.update(host_s=time.perf_counter() - t0, host_queries=len(pick))
    out['host_ms_per_query'] = out['host_s'] * 1e3 / len(pick)
    out['host_equals_kernel'] = bool(np.array_equal(hi, oi.cpu().numpy()[pick]) and np.array_equal(hs, os_.cpu().numpy()[pick]))
    # the composed torch route on the same queries
    try:
        W = itemknn.weight_matrix(idx.cpu().numpy(), nbr_w, I)
        WT = sp.coo_matrix(W.T)
        Wt = torch.sparse_coo_tensor(torch.from_numpy(np.stack([WT.row, WT.col]).astype(np.int64)), torch.from_numpy((WT.data / itemknn.SCALE).astype(np.float32)),
                                     size=(I, I)).coalesce().cuda()
        qd = torch.from_numpy(q_ids).cuda()
        cdeg = (crp[1:] - crp[:-1])

        def composed():
            lists = []
            for b in range(0, len(q_ids), a.chunk):
                q = qd[b:b + a.chunk]
                d = cdeg[q]
                src = (crp[q][:, None] + torch.arange(int(d.max()) if q.numel() else 0, device='cuda')[None, :])
                ok = torch.arange(src.shape[1], device='cuda')[None, :] < d[:, None]
                items = cci[src.clamp_max(cci.numel() - 1)].long()
                B = torch.zeros((I, q.numel()), dtype=torch.float32, device='cuda')                  # the chunk's profiles, transposed
                cols = torch.arange(q.numel(), device='cuda')[:, None].expand_as(items)
                B[items[ok], cols[ok]] = 1.0
                S = torch.sparse.mm(Wt, B)
                S[items[ok], cols[ok]] = float('-inf')
                lists.append(torch.topk(S, min(N, I), dim=0)[1].T)
            return torch.cat(lists)
        out['composed_ms'] = events_ms(composed, max(2, a.reps // 2))
        out['composed_queries'] = len(q_ids)
        out['composed_lists_equal_to_kernel_share'] = float((composed() == oi.long()).all(1).float().mean())
        del Wt
    except Exception as e:                                  # a yardstick only: a torch build without the sparse product still measures the rest
        out['composed_ms'] = None
        out['composed_error'] = '%s: %s' % (type(e).__name__, str(e)[:200])
    torch.cuda.empty_cache()
    return out


def victims(a):
    import torch
    from arlib_amd import detect
    from arlib_amd.util.tool import seedSet
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.metrics import TargetRankMetric
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    from arlib_amd.attack.Black.BandwagonAttack import BandwagonAttack
    from arlib_amd.recommender.GMF import GMF
    from arlib_amd.recommender import ItemKNN
    seedSet(a.seed)
    data, held = clean_data(DataLoader)
    atk_args = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)

    def read(d, target_names):
        res = {}
        for model in ('GMF', 'ItemKNN'):
            args = SimpleNamespace(dataset=d.dataName if hasattr(d, 'dataName') else 'ml-100k', data_path='', training_data='', val_data='', test_data='',
                                   model_name=model, maxEpoch=a.epochs, batch_size=2048, emb_size=a.dim, n_layers=2, reg=1e-4, lRate=0.005, seed=a.seed,
                                   topK='50', knn_k=a.k)
            seedSet(a.seed)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rec = (GMF if model == 'GMF' else ItemKNN)(args, d)
                rec.train()
            m = TargetRankMetric(rec, [d.item[n] for n in target_names], top=[50], mask_train=True)
            res[model] = dict(hitRate50=m.hitRate()[0], ER50=m.exposure()[0], mean_rank=m.meanRank(), recall50=rec.bestPerformance[1]['Recall'],
                              train_and_read_s=round(time.perf_counter() - t0, 2))
            del rec
            torch.cuda.empty_cache()
        return res
    target_names, runs = None, []
    for cls in (RandomAttack, BandwagonAttack):
        seedSet(a.seed)
        atk = cls(atk_args, data)
        if target_names is None:
            target_names = [data.id2item[t] for t in atk.targetItem]
            runs.append(dict(attack='none', users=data.user_num, **read(data, target_names)))
            print(json.dumps(runs[-1]), flush=True)
        atk.targetItem = [data.item[n] for n in target_names]                    # the same five targets for every attack
        poison = sp.csr_matrix(atk.posionDataAttack())
        U, F = data.user_num, poison.shape[0] - data.user_num
        feats = detect.profile_features(poison, k=25, measure='cosine', device='cuda')
        kept, reduced = detect.sanitize(poison, feats['degsim'], F)
        out = dict(attack=cls.__name__, users=U, fake_users=F, dropped_fake=int(F - (kept >= U).sum()))
        for label, mat, ids in (('poisoned', poison, np.arange(U + F)), ('sanitized', reduced, kept)):
            out[label] = read(loader_of(DataLoader, data, mat, ids, held, label + '_ml-100k'), target_names)
        print(json.dumps(out), flush=True)
        runs.append(out)
    return dict(seed=a.seed, attack=vars(atk_args), targets=target_names, epochs=a.epochs, dim=a.dim, knn_k=a.k, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--subset', type=int, default=32768)
    ap.add_argument('--full-limit-s', type=float, default=60.0)
    ap.add_argument('--host-rows', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--skip-cfg2', action='store_true')
    ap.add_argument('--skip-victims', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'itemknn_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('itemknn_bench: needs a GPU (a time taken anywhere else says nothing)')
    out = dict(tool='tools/itemknn_bench.py', device=torch.cuda.get_device_name(0), reps=a.reps, subset=a.subset, full_limit_s=a.full_limit_s,
               timing='device events around the call, one warm-up, median / min / max of reps; host_s and lists_ms one run on the host clock')
    out['ml1m_shape'] = shape(graph(6040, 3706, 165.6), a, 'ml-1M')
    print(json.dumps(out['ml1m_shape']), flush=True)
    if not a.skip_cfg2:
        out['cfg2'] = shape(graph(1_000_000, 100_000, 32.0), a, 'cfg2')
        print(json.dumps(out['cfg2']), flush=True)
    if not a.skip_victims:
        out['victims'] = victims(a)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The exact user-kNN scoring op (arlib_amd/userknn.py, the user side of csrc/arl_itemknn.hip) at ml-1M's shape (6 040 x 3 706, SYN-v1 pairs at
ml-1M's mean degree) and at cfg2's (SYN-v1, 1 M users x 100 K items), and the UserKNN victim beside ItemKNN under Random and Bandwagon poisoning
on ml-100k.  Prints one JSON line per part and writes profiles/userknn_bench.json.

    python tools/userknn_bench.py [--reps 5] [--k 50] [--n 50] [--subset 32768] [--full-limit-s 60] [--host-rows 256] [--skip-cfg2] [--skip-victims]

Per shape (the lists are neighbours.cooccur_topk on the matrix itself, all rows, cosine weights; every profile is masked, N = --n):
  lists_ms       cooccur_topk(route='kernel') on the user side plus knn_weights, host clock, one run;
  plan_ms        the wrapper's preparation on the device (canonical rows, the summed degrees of every user's live neighbours; host clock
                 around a synchronise);
  kernel_ms      arl_userknn_score_topk_i64 alone on that plan (device events; median, min, max of --reps after one warm-up), without targets
                 and with five; entries = the neighbour entries the kernel reads (the degrees of the queries' live neighbours, each once; the
                 chunk re-read at a tile seam is not counted);
  tile_sweep_ms  the kernel without targets at half the default tile, the default and the largest tile;
  call_ms        userknn.uknn_score_topk(route='kernel') as a whole, on device inputs;
  host_s         userknn.uknn_score_topk_host on --host-rows of the queries, host clock, one run; and that the integers are equal;
  composed_ms    torch.sparse.mm of the fp32 weight matrix of --chunk query rows with X (dense at ml-1M's shape, sparse past --dense-limit-bytes),
                 the profile's items set to -inf, torch.topk.  A timing yardstick only: its fp32 sums and its order among ties are not the
                 contract's; the share of rows whose list equals the kernel's is reported.
At cfg2 the kernel is timed on --subset random queries (a test-sized query set) first, and on all users only when that predicts at most
--full-limit-s seconds; the composed route is timed on the same subset.

The victims: ml-100k (tests/golden/ml100k_data.npz), Random and Bandwagon at the reference's default budget (1 % fake users, five unpopular
targets), a UserKNN and an ItemKNN victim fitted on the clean data, on the poisoned data and on the data after detect.sanitize dropped the F
users with the largest degsim, each read with TargetRankMetric (HitRate@50, ER@50, mean rank of the targets, training items masked).  Beside the
poisoned UserKNN: the mean neighbour_share of the fake ids over the real users (how much of a real user's neighbourhood weight the fakes hold)
and the AUC of detect.profile_features' knn_indegree at k = 25 (the sanitising step's) and at the victim's k.  A measurement to report as it
comes out, not a test and not a claim."""
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
    from arlib_amd import _lib, itemknn, neighbours, ops, userknn
    U, I = X.shape
    k, N = a.k, a.n
    out = dict(shape=name, users=U, items=I, nnz=int(X.nnz), k=k, N=N, tile_items=userknn.UKNN_DEFAULT_TILE_ITEMS,
               tiles=-(-I // userknn.UKNN_DEFAULT_TILE_ITEMS), max_profile=int(np.diff(X.indptr).max()))
    rp, ci = torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    idx, cnt, deg = neighbours.cooccur_topk(rp, ci, U, I, k, 'cosine', route='kernel')
    nbr_w = itemknn.knn_weights(idx, cnt, deg, 'cosine')
    out['lists_ms'] = (time.perf_counter() - t0) * 1e3
    ni, nw = idx.contiguous(), torch.from_numpy(nbr_w).cuda()
    del cnt

    def plan():
        crp, cci, _, d = neighbours._canonical(rp, ci, U, I)
        weight = torch.where(ni >= 0, d[ni.clamp(min=0).long()], torch.zeros_like(ni, dtype=torch.int64)).sum(1)
        return crp, cci, weight
    out['plan_ms'] = host_ms(plan, a.reps)
    crp, cci, weight = plan()
    L, P = _lib.lib(), ops._ptr
    tg = torch.sort(torch.from_numpy(np.random.RandomState(2).choice(I, 5, replace=False).astype(np.int32))).values.cuda()
    tcol = torch.arange(5, dtype=torch.int32, device='cuda')

    def kernel(rows, T, tile=0):
        Q = U if rows is None else rows.numel()
        wq = weight if rows is None else weight[rows.long()]
        order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
        oi, os_ = torch.empty((Q, N), dtype=torch.int32, device='cuda'), torch.empty((Q, N), dtype=torch.int64, device='cuda')
        rk = torch.empty((Q, max(T, 1)), dtype=torch.int32, device='cuda')
        run = lambda: _lib.check(L.arl_userknn_score_topk_i64(P(crp), P(cci), U, I, P(ni), P(nw), k, P(rows), Q, N, 1, P(tg) if T else None,
                                                              P(tcol) if T else None, T, P(order), tile, P(oi), P(os_), P(rk) if T else None,
                                                              ops._stream()), 'arl_userknn_score_topk_i64')
        return run, oi, os_, float(wq.sum())
    rng = np.random.RandomState(1)
    sub = None
    if U > a.subset:
        sub = torch.from_numpy(np.sort(rng.choice(U, a.subset, replace=False)).astype(np.int32)).cuda()
        run, oi, os_, ent = kernel(sub, 0)
        t = events_ms(run, max(2, a.reps // 2))
        out.update(subset_queries=a.subset, subset_kernel_ms=t, subset_entries=ent, subset_gentries_per_s=ent / t[0] / 1e6,
                   subset_kernel_5_targets_ms=events_ms(kernel(sub, 5)[0], max(2, a.reps // 2)), full_kernel_ms_predicted_from_subset=t[0] * U / a.subset,
                   subset_call_ms=events_ms(lambda: userknn.uknn_score_topk(rp, ci, U, I, ni, nw, N, rows=sub, mask_profile=True, route='kernel'), 2))
        if t[0] * U / a.subset > a.full_limit_s * 1e3:
            out['kernel_ms'] = None
            out['note'] = 'all users not timed: the subset predicts more than --full-limit-s = %g s' % a.full_limit_s
    if 'kernel_ms' not in out:
        run, oi_all, os_all, ent = kernel(None, 0)
        t = events_ms(run, a.reps if sub is None else 2)
        out.update(kernel_ms=t, entries=ent, gentries_per_s=ent / t[0] / 1e6, kernel_ms_per_query=t[0] / U)
        if sub is None:
            out['kernel_5_targets_ms'] = events_ms(kernel(None, 5)[0], a.reps)
            out['call_ms'] = events_ms(lambda: userknn.uknn_score_topk(rp, ci, U, I, ni, nw, N, mask_profile=True, route='kernel'), a.reps)
            oi, os_ = oi_all, os_all
        else:
            del oi_all, os_all
    # the tile size: the default (80 KiB, two workgroups per CU) against half of it and the largest (160 KiB, one workgroup per CU)
    out['tile_sweep_ms'] = {str(t): events_ms(kernel(sub, 0, t)[0], max(2, a.reps // 2))
                            for t in (userknn.UKNN_DEFAULT_TILE_ITEMS // 2, userknn.UKNN_DEFAULT_TILE_ITEMS, userknn.UKNN_MAX_TILE_ITEMS)}
    q_ids = np.arange(U) if sub is None else sub.cpu().numpy().astype(np.int64)
    # the host route on --host-rows of the timed queries
    pick = np.sort(rng.choice(len(q_ids), min(a.host_rows, len(q_ids)), replace=False))
    idx_h = idx.cpu().numpy()
    t0 = time.perf_counter()
    hi, hs, _ = userknn.uknn_score_topk_host(X, idx_h, nbr_w, N, q_ids[pick], True)
    out.update(host_s=time.perf_counter() - t0, host_queries=len(pick))
    out['host_ms_per_query'] = out['host_s'] * 1e3 / len(pick)
    out['host_equals_kernel'] = bool(np.array_equal(hi, oi.cpu().numpy()[pick]) and np.array_equal(hs, os_.cpu().numpy()[pick]))
    # the composed torch route on the same queries
    try:
        dense = 4 * U * I <= a.dense_limit_bytes
        coo = sp.coo_matrix(X)
        Xs = torch.sparse_coo_tensor(torch.from_numpy(np.stack([coo.row, coo.col]).astype(np.int64)), torch.ones(coo.nnz, dtype=torch.float32),
                                     size=(U, I)).coalesce().cuda()
        Xd = Xs.to_dense() if dense else None
        qd = torch.from_numpy(q_ids).cuda()
        cdeg = (crp[1:] - crp[:-1])
        wf = torch.where(ni >= 0, nw.float() / itemknn.SCALE, torch.zeros((), device='cuda'))

        def composed():
            lists = []
            for b in range(0, len(q_ids), a.chunk):
                q = qd[b:b + a.chunk]
                live = ni[q] >= 0
                r = torch.arange(q.numel(), device='cuda')[:, None].expand(-1, k)[live]
                Wq = torch.sparse_coo_tensor(torch.stack([r, ni[q][live].long()]), wf[q][live], size=(q.numel(), U)).coalesce()
                S = torch.sparse.mm(Wq, Xd) if dense else torch.sparse.mm(Wq, Xs).to_dense()
                d = cdeg[q]
                src = (crp[q][:, None] + torch.arange(int(d.max()) if q.numel() else 0, device='cuda')[None, :])
                ok = torch.arange(src.shape[1], device='cuda')[None, :] < d[:, None]
                items = cci[src.clamp_max(cci.numel() - 1)].long()
                rows_ = torch.arange(q.numel(), device='cuda')[:, None].expand_as(items)
                S[rows_[ok], items[ok]] = float('-inf')
                lists.append(torch.topk(S, min(N, I), dim=1)[1])
            return torch.cat(lists)
        out['composed_x'] = 'dense' if dense else 'sparse'
        out['composed_ms'] = events_ms(composed, max(2, a.reps // 2))
        out['composed_queries'] = len(q_ids)
        out['composed_lists_equal_to_kernel_share'] = float((composed() == oi.long()).all(1).float().mean())
        del Xs, Xd
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
    from arlib_amd.util.metrics import DetectionMetric, TargetRankMetric
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    from arlib_amd.attack.Black.BandwagonAttack import BandwagonAttack
    from arlib_amd.recommender import ItemKNN, UserKNN
    seedSet(a.seed)
    data, held = clean_data(DataLoader)
    atk_args = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)

    def read(d, target_names, fake_names=()):
        res = {}
        for model in ('UserKNN', 'ItemKNN'):
            args = SimpleNamespace(dataset=d.dataName if hasattr(d, 'dataName') else 'ml-100k', data_path='', training_data='', val_data='', test_data='',
                                   model_name=model, maxEpoch=1, batch_size=2048, emb_size=64, n_layers=2, reg=1e-4, lRate=0.005, seed=a.seed,
                                   topK='50', knn_k=a.k)
            seedSet(a.seed)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rec = (UserKNN if model == 'UserKNN' else ItemKNN)(args, d)
                rec.train()
            m = TargetRankMetric(rec, [d.item[n] for n in target_names], top=[50], mask_train=True)
            res[model] = dict(hitRate50=m.hitRate()[0], ER50=m.exposure()[0], mean_rank=m.meanRank(), recall50=rec.bestPerformance[1]['Recall'],
                              train_and_read_s=round(time.perf_counter() - t0, 2))
            if model == 'UserKNN' and len(fake_names):
                share = rec.neighbour_share(fake_names)
                real = np.array([d.user[u] for u in d.user if u not in set(fake_names)], np.int64)
                res[model]['fake_neighbour_share_mean_over_real_users'] = float(share[real].mean())
                res[model]['real_users_with_a_fake_neighbour'] = int((share[real] > 0).sum())
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
        feats = detect.profile_features(poison, k=25, measure='cosine', device='cuda')               # tools/itemknn_bench.py's sanitising step
        kept, reduced = detect.sanitize(poison, feats['degsim'], F)
        at_k = detect.profile_features(poison, k=a.k, measure='cosine', device='cuda')              # the victim's own neighbourhoods
        auc = lambda f: DetectionMetric(f['knn_indegree'], np.arange(U, U + F)).auc()
        out = dict(attack=cls.__name__, users=U, fake_users=F, dropped_fake=int(F - (kept >= U).sum()), knn_indegree_auc_k25=auc(feats),
                   knn_indegree_auc_at_knn_k=auc(at_k))
        for label, mat, ids in (('poisoned', poison, np.arange(U + F)), ('sanitized', reduced, kept)):
            fake_names = ['fake%d' % (r - U) for r in ids.tolist() if r >= U]
            out[label] = read(loader_of(DataLoader, data, mat, ids, held, label + '_ml-100k'), target_names, fake_names)
        print(json.dumps(out), flush=True)
        runs.append(out)
    return dict(seed=a.seed, attack=vars(atk_args), targets=target_names, knn_k=a.k, runs=runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--k', type=int, default=50)
    ap.add_argument('--n', type=int, default=50)
    ap.add_argument('--subset', type=int, default=32768)
    ap.add_argument('--full-limit-s', type=float, default=60.0)
    ap.add_argument('--host-rows', type=int, default=256)
    ap.add_argument('--chunk', type=int, default=4096)
    ap.add_argument('--dense-limit-bytes', type=int, default=1 << 30)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--skip-cfg2', action='store_true')
    ap.add_argument('--skip-victims', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'userknn_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('userknn_bench: needs a GPU (a time taken anywhere else says nothing)')
    out = dict(tool='tools/userknn_bench.py', device=torch.cuda.get_device_name(0), reps=a.reps, subset=a.subset, full_limit_s=a.full_limit_s,
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

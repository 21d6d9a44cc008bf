#!/usr/bin/env python3
"""Can the injected profiles be told apart from real ones?  ml-100k (tests/golden/ml100k_data.npz), Random, Bandwagon and AUSH at the reference's
default budget (1 % fake users, five unpopular targets, the same five for every attack), fixed seeds.  The attack arguments' Epoch / innerEpoch /
outerEpoch are read by the surrogate-based attacks only: AUSH trains its GAN for its own default length, 50 rounds of 25 discriminator and 25
generator steps (BiLevelOptimizationEpoch, posionDataAttack's epoch1 / epoch2), whatever they say.

    python tools/detect_bench.py [--k 25 --measure cosine --epochs 30 --dim 64 --out profiles/detect_bench.json]

Per attack: AUC and precision@F (F = the number of fake users) of the two neighbour features of arlib_amd.detect.profile_features, degsim and
knn_indegree, read as "higher = more suspicious", with the neighbour lists from the kernel (device 'cuda'); for contrast the same two figures of
length_var and mean_popularity.  For Bandwagon also the data-level defence: a GMF victim trained on the poisoned data as it is, and on the data
after detect.sanitize dropped the F top-scored users (by degsim), each read with TargetRankMetric's HitRate@50 and ER@50 of the targets; how many
of the dropped users were fake is stated beside it.  A measurement to report as it comes out, not a test and not a claim."""
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
import numpy as np                            # noqa: E402
import scipy.sparse as sp                     # noqa: E402


def clean_data(DataLoader):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ml100k_data.npz'))
    held = [(g[n + '_u'], g[n + '_i'], g[n + '_r']) for n in ('val', 'test')]
    return DataLoader.from_arrays((g['train_u'], g['train_i'], g['train_r']), held[0], held[1], dataName='ml-100k', array_native=False), held


def loader_of(DataLoader, data, matrix, row_ids, held, name):
    """A DataLoader over the rows `row_ids` (ids into the attack's (U + F) x I matrix) of `matrix`: real users keep their raw ids, fake users get
    new ones; the held-out splits keep the pairs of the users that remain."""
    U = data.user_num
    m = sp.coo_matrix(matrix)
    names = [data.id2user[r] if r < U else 'fake%d' % (r - U) for r in row_ids.tolist()]
    users = [names[r] for r in m.row.tolist()]
    items = [data.id2item[c] for c in m.col.tolist()]
    left = set(names)
    cut = []
    for u, i, r in held:
        keep = np.array([str(x) in left for x in np.asarray(u).tolist()], bool)
        cut.append((np.asarray(u)[keep], np.asarray(i)[keep], np.asarray(r)[keep]))
    return DataLoader.from_arrays((users, items, np.ones(len(users))), cut[0], cut[1], dataName=name, array_native=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=25)
    ap.add_argument('--measure', default='cosine')
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'detect_bench.json'))
    a = ap.parse_args()

    import torch
    from arlib_amd import detect
    from arlib_amd.util.tool import seedSet
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.metrics import DetectionMetric, TargetRankMetric
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    from arlib_amd.attack.Black.BandwagonAttack import BandwagonAttack
    from arlib_amd.attack.Gray.AUSH import AUSH
    from arlib_amd.recommender.GMF import GMF
    if not torch.cuda.is_available():
        sys.exit('detect_bench: needs a GPU (the neighbour kernel, AUSH and the victims run on the device)')
    seedSet(a.seed)
    data, held = clean_data(DataLoader)
    atk_args = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)
    target_names, runs = None, []
    for cls in (RandomAttack, BandwagonAttack, AUSH):
        seedSet(a.seed)
        atk = cls(atk_args, data)
        if target_names is None:
            target_names = [data.id2item[t] for t in atk.targetItem]
        atk.targetItem = [data.item[n] for n in target_names]                    # the same five targets for every attack
        t0 = time.perf_counter()
        poison = sp.csr_matrix(atk.posionDataAttack())
        attack_s = time.perf_counter() - t0
        U, F = data.user_num, poison.shape[0] - data.user_num
        fake = np.arange(U, U + F)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        feats = detect.profile_features(poison, k=a.k, measure=a.measure, device='cuda')
        features_s = time.perf_counter() - t0
        host = detect.profile_features(poison, k=a.k, measure=a.measure)
        out = dict(attack=cls.__name__, users=U, fake_users=F, items=poison.shape[1], k=a.k, measure=a.measure, attack_s=round(attack_s, 2),
                   features_s=round(features_s, 4), kernel_features_equal_host=bool(all(np.array_equal(feats[n], host[n]) for n in feats)),
                   fake_profile_length=[int(x) for x in np.diff(poison.indptr)[fake]], real_profile_length_mean=float(np.diff(poison.indptr)[:U].mean()))
        for name, s in feats.items():
            m = DetectionMetric(s, fake)
            out[name] = dict(auc=m.auc(), precision_at_F=m.precision_at(F), recall_at_F=m.recall_at(F), fake_mean=float(s[fake].mean()), real_mean=float(s[:U].mean()))
        if cls is BandwagonAttack:
            targets_of = lambda d: [d.item[n] for n in target_names]
            kept, reduced = detect.sanitize(poison, feats['degsim'], F)
            out['sanitize'] = dict(dropped=F, dropped_fake=int(F - (kept >= U).sum()), dropped_real=int(U - (kept < U).sum()))
            for label, mat, ids in (('poisoned', poison, np.arange(U + F)), ('sanitized', reduced, kept)):
                d = loader_of(DataLoader, data, mat, ids, held, label + '_ml-100k')
                args = SimpleNamespace(dataset=label, data_path='', training_data='', val_data='', test_data='', model_name='GMF', maxEpoch=a.epochs, batch_size=2048,
                                       emb_size=a.dim, n_layers=2, reg=1e-4, lRate=0.005, seed=a.seed, topK='50')
                seedSet(a.seed)
                with contextlib.redirect_stdout(io.StringIO()):
                    rec = GMF(args, d)
                    rec.train()
                m = TargetRankMetric(rec, targets_of(d), top=[50], mask_train=True)
                out['sanitize'][label] = dict(users=d.user_num, hitRate50=m.hitRate()[0], ER50=m.exposure()[0], mean_rank=m.meanRank())
                del rec
                torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)
        runs.append(out)
    with open(a.out, 'w') as fh:
        json.dump({'tool': 'tools/detect_bench.py', 'seed': a.seed, 'attack': vars(atk_args), 'targets': target_names, 'epochs': a.epochs, 'dim': a.dim, 'runs': runs}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

#!/usr/bin/env python3
"""The robustness comparison DESIGN.md section 10 left open: defended against undefended victims under the data-only shilling attacks, read with the
full-ranking metrics of util.metrics.TargetRankMetric.  ml-100k (tests/golden/ml100k_data.npz), fixed seeds.

    python tools/robustness_bench.py [--epochs 30 --dim 64 --layers 2 --out profiles/robustness_bench.json]

Victims: GMF and LightGCN, and APR on each encoder (apr_encoder 'mf' / 'lightgcn').  Data: clean, and the output of RandomAttack and BandwagonAttack
(1 % fake users, the reference's defaults: five unpopular targets, the same five for every run).  Every victim is trained from the same seed on every
data set.  Per run: mean rank, MRR and ER@{50, 500} of the targets over all users with and without the users' training interactions masked
(masked, a fake user's pairs drop out: it already has every target), and AttackMetric's HitRate@50 for contrast.  A measurement to report as it
comes out, not a test and not a claim; prints one JSON line per run and writes them all to --out."""
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

VICTIMS = (('GMF', 'GMF', {}), ('LightGCN', 'LightGCN', {}), ('APR-mf', 'APR', {'apr_encoder': 'mf'}), ('APR-lightgcn', 'APR', {'apr_encoder': 'lightgcn'}))


def clean_data(DataLoader):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ml100k_data.npz'))
    held = [(g[n + '_u'], g[n + '_i'], g[n + '_r']) for n in ('val', 'test')]
    return DataLoader.from_arrays((g['train_u'], g['train_i'], g['train_r']), held[0], held[1], dataName='ml-100k', array_native=False), held


def poisoned_data(DataLoader, data, poison, held, name):
    """A DataLoader over the attack's rating matrix: real users keep their raw ids, fake users get new ones; held-out splits unchanged."""
    m = sp.coo_matrix(poison)
    U = data.user_num
    users = [data.id2user[r] if r < U else 'fake%d' % (r - U) for r in m.row.tolist()]
    items = [data.id2item[c] for c in m.col.tolist()]
    return DataLoader.from_arrays((users, items, np.ones(len(users))), held[0], held[1], dataName=name, array_native=False)


def victim_class(model):
    if model == 'APR':
        from arlib_amd.recommender import APR
        return APR
    mod = __import__('arlib_amd.recommender.' + model, fromlist=[model])
    return getattr(mod, model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=30)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--layers', type=int, default=2)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'robustness_bench.json'))
    a = ap.parse_args()

    import torch
    from arlib_amd.util.tool import seedSet
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.metrics import AttackMetric, TargetRankMetric
    from arlib_amd.attack.Black.RandomAttack import RandomAttack
    from arlib_amd.attack.Black.BandwagonAttack import BandwagonAttack
    if not torch.cuda.is_available():
        sys.exit('robustness_bench: needs a GPU (the victims train on the device)')
    seedSet(a.seed)
    data, held = clean_data(DataLoader)
    atk_args = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)
    target_names = None
    sets = [('clean', data)]
    for cls in (RandomAttack, BandwagonAttack):
        seedSet(a.seed)
        atk = cls(atk_args, data)
        if target_names is None:
            target_names = [data.id2item[t] for t in atk.targetItem]
        atk.targetItem = [data.item[n] for n in target_names]                    # the same five targets for every attack
        sets.append((cls.__name__, poisoned_data(DataLoader, data, atk.posionDataAttack(), held, cls.__name__ + '_ml-100k')))
    runs = []
    for set_name, d in sets:
        targets = [d.item[n] for n in target_names]
        for label, model, extra in VICTIMS:
            args = SimpleNamespace(dataset=d.dataName if hasattr(d, 'dataName') else set_name, data_path='', training_data='', val_data='', test_data='', model_name=model,
                                   maxEpoch=a.epochs, batch_size=2048, emb_size=a.dim, n_layers=a.layers, reg=1e-4, lRate=0.005, seed=a.seed, topK='50', **extra)
            seedSet(a.seed)
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                rec = victim_class(model)(args, d)
                rec.train()
            train_s = time.perf_counter() - t0
            out = dict(data=set_name, victim=label, users=d.user_num, items=d.item_num, train_s=round(train_s, 2), targets=target_names,
                       target_train_count=[int(c) for c in np.asarray(sp.csr_matrix(d.matrix())[:, targets].sum(0)).ravel()])
            for masked in (False, True):
                m = TargetRankMetric(rec, targets, top=[50, 500], mask_train=masked)
                er = m.exposure()
                out['masked' if masked else 'unmasked'] = dict(mean_rank=m.meanRank(), MRR=m.MRR(), ER50=er[0], ER500=er[1], hitRate50=m.hitRate()[0],
                                                               valid_pairs=int((m.ranks() >= 0).sum()))
            out['AttackMetric_hitRate50'] = AttackMetric(rec, targets, [50]).hitRate()[0]
            print(json.dumps(out), flush=True)
            runs.append(out)
            del rec
            torch.cuda.empty_cache()
    with open(a.out, 'w') as fh:
        json.dump({'tool': 'tools/robustness_bench.py', 'epochs': a.epochs, 'dim': a.dim, 'layers': a.layers, 'seed': a.seed, 'attack': vars(atk_args), 'runs': runs}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

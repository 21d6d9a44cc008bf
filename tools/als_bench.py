#!/usr/bin/env python3
"""The ALS row solve (csrc/arl_als.hip) against the composed torch route, a whole sweep, the effect of split_len, and iALS against GMF.  Prints one JSON
line per leg and writes them all to profiles/als_bench.json.

    python tools/als_bench.py [--legs rows,crossover,sweep,split,converge --shapes ml1m,cfg2 --dims 64,128 --reps 5 --out profiles/als_bench.json]

Shapes are SYN-v1 graphs (util/synthetic.py) of ml-1M's size (6 040 x 3 706, mean degree 165.6) and cfg2's (1 000 000 x 100 000, mean degree 32).
Legs:
  rows      one half-sweep's row solve, user side and item side: kernel and composed on the same inputs.  A timed window is `inner` calls between two
            device synchronises on the host clock (inner chosen so that a window lasts about 0.2 s); the two routes' windows ALTERNATE, --reps of
            each after a warm-up; minimum, median and maximum per call.  Peak device memory above the inputs.  The kernel's share of the exact-fp32
            MFMA floor: the flop it issues (the lower-triangular 16 x 16 tiles of sum w y y^T, 2 * 256 * tiles per entry) and the full 2 nnz d^2,
            each against the fp32 matrix peak.  Both routes' row-wise errors against float64 on the first 128 rows and on the 8 longest.
  crossover the first 1 .. 4 096 user rows at ml-1M's shape, kernel against composed: what route = 'auto' goes by.
  sweep     gram + user rows + gram + item rows at cfg2 on the kernel route.
  split     the item side (the hub rows) at several split_len.
  converge  iALS sweeps and wall time to reach GMF's best recall@k on a SYN-v1 set with a held-out item per user, beside GMF's own epochs and time.
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
from arlib_amd import als                     # noqa: E402
from arlib_amd.util import synthetic          # noqa: E402

SHAPES = {'ml1m': dict(U=6040, I=3706, deg=165.6), 'cfg2': dict(U=1_000_000, I=100_000, deg=32.0)}
PEAK_TFLOPS = 157.3                           # fp32 matrix peak of the MI355X
ALPHA, REG = 10.0, 0.1


def window(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner


def alternating(fns, reps):
    inn = {}
    for name, fn in fns.items():
        fn()
        inn[name] = max(1, min(200, int(0.2 / max(window(fn, 1), 1e-5))))
    got = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            got[name].append(window(fn, inn[name]))
    return {name: dict(min_s=min(v), median_s=statistics.median(v), max_s=max(v), calls_per_window=inn[name]) for name, v in got.items()}


def peak_above(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def graph(name):
    """{'user': csr, 'item': csr} int32 device CSRs of the shape's SYN-v1 graph."""
    S = SHAPES[name]
    p = np.asarray(synthetic.syn_v1_pairs_native(S['U'], S['I'], S['deg'], 2018))
    out = {}
    for side, (r, c, n) in (('user', (p[:, 0], p[:, 1], S['U'])), ('item', (p[:, 1], p[:, 0], S['I']))):
        order = np.lexsort((c, r))
        rowptr = np.zeros(n + 1, np.int64)
        rowptr[1:] = np.cumsum(np.bincount(r, minlength=n))
        out[side] = (torch.from_numpy(rowptr.astype(np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(c[order]).astype(np.int32)).cuda())
    return out


def row_err(got, want):
    nz = want.norm(dim=1) > 0
    return float(((got.double()[nz] - want[nz]).norm(dim=1) / want[nz].norm(dim=1)).max())


def tables(name, d):
    S = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(d)
    return {'user': 0.1 * torch.randn(S['U'], d, device='cuda', generator=g), 'item': 0.1 * torch.randn(S['I'], d, device='cuda', generator=g)}


def run_rows(name, G_csr, d, reps, composed=True):
    T = tables(name, d)
    nt = d // 16
    lines = []
    for side, other in (('user', 'item'), ('item', 'user')):
        Y, csr = T[other], G_csr[side]
        G = als.gram(Y)
        deg = (csr[0][1:] - csr[0][:-1]).long()
        nnz, n_solve = int(csr[1].numel()), int(deg.numel())
        out = dict(leg='rows', shape=name, side=side, rows=n_solve, other_rows=int(Y.shape[0]), dim=d, nnz=nnz, longest_row=int(deg.max()), mean_row=nnz / n_solve)
        kern = lambda: als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, check_range=False)
        fns = {'kernel': kern}
        if composed:
            fns['composed'] = lambda: als.als_solve_rows_composed(Y, G, csr, ALPHA, REG)
        t = alternating(fns, reps)
        out['time'] = t
        out['gram_s'] = alternating({'gram': lambda: als.gram(Y)}, reps)['gram']['median_s']
        out['kernel_peak_bytes'] = peak_above(kern)
        if composed:
            out['speedup_median'] = t['composed']['median_s'] / t['kernel']['median_s']
            out['composed_peak_bytes'] = peak_above(fns['composed'])
        else:
            out['composed'] = 'not measured'
        out['stack_of_A_bytes_fp32'] = 4 * n_solve * d * d
        out['issued_flop'] = 2.0 * 256 * (nt * (nt + 1) // 2) * nnz
        out['full_flop'] = 2.0 * nnz * d * d
        out['issued_mfma_floor_s'] = out['issued_flop'] / (PEAK_TFLOPS * 1e12)
        out['full_mfma_floor_s'] = out['full_flop'] / (PEAK_TFLOPS * 1e12)
        out['kernel_share_of_issued_mfma_floor'] = out['issued_mfma_floor_s'] / t['kernel']['median_s']
        out['kernel_share_of_full_mfma_floor'] = out['full_mfma_floor_s'] / t['kernel']['median_s']
        sub = torch.cat([torch.arange(min(128, n_solve), device='cuda'), torch.topk(deg, min(8, n_solve))[1]]).to(torch.int32)
        want = als.als_solve_rows_composed(Y.double(), G, csr, ALPHA, REG, rows=sub)
        out['error_rows'] = int(sub.numel())
        out['kernel_row_err'] = row_err(als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, rows=sub), want)
        out['composed_row_err'] = row_err(als.als_solve_rows_composed(Y, G, csr, ALPHA, REG, rows=sub), want)
        lines.append(out)
    return lines


def run_crossover(name, G_csr, d, reps):
    """The user side's first n rows, n from 1 up: where does the kernel's call stop losing to the composed route's (what route='auto' goes by)."""
    T = tables(name, d)
    Y, csr = T['item'], G_csr['user']
    G = als.gram(Y)
    out = dict(leg='crossover', shape=name, side='user', dim=d, by_rows={})
    for n in (1, 8, 64, 512, 4096):
        if n > csr[0].numel() - 1:
            break
        sub = torch.arange(n, dtype=torch.int32, device='cuda')
        t = alternating({'kernel': lambda: als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, rows=sub, check_range=False),
                         'composed': lambda: als.als_solve_rows_composed(Y, G, csr, ALPHA, REG, rows=sub)}, reps)
        out['by_rows'][str(n)] = dict(kernel_median_s=t['kernel']['median_s'], composed_median_s=t['composed']['median_s'],
                                      speedup_median=t['composed']['median_s'] / t['kernel']['median_s'])
    return out


def run_sweep(name, G_csr, d, reps):
    T = tables(name, d)

    def sweep():
        X = als.als_solve_rows_kernel(T['item'], als.gram(T['item']), G_csr['user'], ALPHA, REG, check_range=False)
        return als.als_solve_rows_kernel(X, als.gram(X), G_csr['item'], ALPHA, REG, check_range=False)
    t = alternating({'sweep': sweep}, reps)['sweep']
    obj = alternating({'objective': lambda: als.als_objective(T['user'], T['item'], G_csr['user'], ALPHA, REG, check_range=False)}, reps)['objective']
    return dict(leg='sweep', shape=name, dim=d, nnz=int(G_csr['user'][1].numel()), sweep=t, objective=obj, peak_bytes=peak_above(sweep))


def run_split(name, G_csr, d, reps):
    T = tables(name, d)
    Y, csr = T['user'], G_csr['item']
    G = als.gram(Y)
    deg = (csr[0][1:] - csr[0][:-1]).long()
    out = dict(leg='split', shape=name, side='item', dim=d, longest_row=int(deg.max()), mean_row=float(deg.double().mean()), default_split_len=als.default_split_len(), by_split_len={})
    base = als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, check_range=False)
    for s in (512, 2048, 8192, 32768, 2 ** 31 - 1):
        fn = lambda: als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, split_len=s, check_range=False)
        t = alternating({'k': fn}, reps)['k']
        t.update(split_rows=int((deg > s).sum()), peak_bytes=peak_above(fn), max_abs_diff_to_default=float((fn() - base).abs().max()))
        out['by_split_len'][str(s)] = t
    return out


def run_converge(d, users, items, max_epochs, max_sweeps):
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender import iALS
    from arlib_amd.recommender.GMF import GMF
    pairs = synthetic.syn_v1_pairs(users, items, mean_deg=32.0, seed=7)
    last = np.r_[pairs[1:, 0] != pairs[:-1, 0], True]                  # the last item of every user is held out where its item keeps training users
    count = np.bincount(pairs[:, 1], minlength=items)
    test = last.copy()
    for k in np.nonzero(test)[0]:
        if count[pairs[k, 1]] > 2:
            count[pairs[k, 1]] -= 1
        else:
            test[k] = False
    one = lambda p: (p[:, 0], p[:, 1], np.ones(len(p)))
    data = DataLoader.from_arrays(one(pairs[~test]), None, one(pairs[test]), dataName='syn', array_native=False)
    args = dict(dataset='syn', maxEpoch=max_epochs, batch_size=2048, emb_size=d, n_layers=0, reg=1e-4, lRate=0.005, seed=2018, topK='20')

    def recall(rec):
        with contextlib.redirect_stdout(io.StringIO()):
            m = rec.test()[1]
        return float([x for x in m if x.startswith('Recall:')][0].split(':')[1])
    out = dict(leg='converge', users=data.user_num, items=data.item_num, train_pairs=len(data.training_data), test_pairs=len(data.test_data), dim=d, k=20)
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        gmf = GMF(SimpleNamespace(model_name='GMF', **args), data)
    curve, spent = [], 0.0
    for e in range(max_epochs):
        torch.cuda.synchronize(); t = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            gmf.train(Epoch=1, evalNum=10 ** 9, optimizer=getattr(gmf, 'optimizer', None))
        torch.cuda.synchronize(); spent += time.perf_counter() - t
        curve.append((e + 1, spent, recall(gmf)))
    best = max(curve, key=lambda c: c[2])
    out['gmf'] = dict(epochs_run=max_epochs, best_recall=best[2], best_epoch=best[0], seconds_to_best=best[1], seconds_all=spent,
                      note='train(Epoch=1) per epoch with the same optimizer; each call includes its own end-of-training bookkeeping', curve=curve[::max(1, max_epochs // 10)])
    seedSet(2018)
    with contextlib.redirect_stdout(io.StringIO()):
        rec = iALS(SimpleNamespace(model_name='iALS', als_route='fused', **args), data)
    rec.model.cuda()
    curve, spent, reached = [], 0.0, None
    for s in range(max_sweeps):
        torch.cuda.synchronize(); t = time.perf_counter()
        rec.half_sweep('user'); rec.half_sweep('item')
        torch.cuda.synchronize(); spent += time.perf_counter() - t
        rec.user_emb, rec.item_emb = rec._detached_forward()
        curve.append((s + 1, spent, recall(rec)))
        if reached is None and curve[-1][2] >= best[2]:
            reached = curve[-1]
    out['ials'] = dict(alpha=rec.als_alpha, reg=rec.als_reg, sweeps_run=max_sweeps, best_recall=max(c[2] for c in curve), curve=curve,
                       sweeps_to_gmf_best=None if reached is None else reached[0], seconds_to_gmf_best=None if reached is None else reached[1])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='rows,crossover,sweep,split,converge')
    ap.add_argument('--shapes', default='ml1m,cfg2')
    ap.add_argument('--dims', default='64,128')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--no-composed-at', default='', help='shape:dim pairs at which the composed route is not timed, comma separated')
    ap.add_argument('--converge-users', type=int, default=6000)
    ap.add_argument('--converge-items', type=int, default=3000)
    ap.add_argument('--converge-epochs', type=int, default=40)
    ap.add_argument('--converge-sweeps', type=int, default=12)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'als_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('als_bench: needs the GPU; nothing here is measured on the CPU')
    legs, dims, skip = a.legs.split(','), [int(x) for x in a.dims.split(',')], set(a.no_composed_at.split(','))
    lines = []

    def emit(x):
        for line in (x if isinstance(x, list) else [x]):
            lines.append(line)
            print(json.dumps(line), flush=True)
    for name in a.shapes.split(','):
        if not {'rows', 'crossover', 'sweep', 'split'} & set(legs):
            break
        g = graph(name)
        for d in dims:
            if 'rows' in legs:
                emit(run_rows(name, g, d, a.reps, composed='%s:%d' % (name, d) not in skip))
            if 'crossover' in legs and name == 'ml1m':
                emit(run_crossover(name, g, d, a.reps))
            if 'sweep' in legs and name == 'cfg2':
                emit(run_sweep(name, g, d, a.reps))
            if 'split' in legs and name == 'cfg2':
                emit(run_split(name, g, d, a.reps))
    if 'converge' in legs:
        emit(run_converge(64, a.converge_users, a.converge_items, a.converge_epochs, a.converge_sweeps))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    prior = []
    if os.path.exists(a.out):                     # legs are measured in several runs: keep the other runs' lines
        with open(a.out) as fh:
            prior = [l for l in json.load(fh).get('legs', []) if not any(l.get('leg') == n.get('leg') and l.get('shape') == n.get('shape') and l.get('dim') == n.get('dim')
                                                                      and l.get('side') == n.get('side') for n in lines)]
    with open(a.out, 'w') as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, alpha=ALPHA, reg=REG, auto_min_rows=als.ALS_AUTO_MIN_ROWS, legs=prior + lines), fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

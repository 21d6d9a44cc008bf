#!/usr/bin/env python3
"""The adjoint of the ALS row solve (csrc/arl_als.hip; arlib_amd/alsgrad.py) against the composed torch route and against the forward solve, the
effect of col_split_len, and one RevAdv outer epoch.  Prints one JSON line per leg and writes them all to profiles/alsgrad_bench.json.

    python tools/alsgrad_bench.py [--legs adjoint,crossover,colsplit,forward,revadv --dims 64,128 --reps 5 --out profiles/alsgrad_bench.json]

Shapes and timing windows are tools/als_bench.py's: SYN-v1 graphs of ml-1M's size and cfg2's; a window is `inner` calls between two device
synchronises on the host clock, the routes' windows alternate, minimum / median / maximum per call.
Legs:
  adjoint   ml-1M, both half-sweeps: als_adjoint_kernel against als_adjoint_composed and against torch autograd through the composed forward (forward
            plus backward, the forward's own time beside it), on the same inputs; peak device memory above the inputs; both routes' errors against
            the float64 composed route.
  crossover the first 1 .. 4 096 user rows at ml-1M's shape and all of them, kernel against composed: what ALSGRAD_AUTO_MIN_ROWS goes by.
  colsplit  the user half at ml-1M's shape (the columns are the items: hub columns) at several col_split_len.
  forward   cfg2, each half: the adjoint kernel against the forward als_solve_rows_kernel of the same half.  The composed route cannot hold the
            shape's gathers in a time worth measuring and is not timed.
  revadv    one RevAdv outer epoch (outer_loss + backward) at ml-1M's shape with the default budget (1 % fake users), fused against composed.
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
from arlib_amd import als, alsgrad            # noqa: E402
from arlib_amd.allpairs import transpose_positives                      # noqa: E402
from als_bench import SHAPES, ALPHA, REG, alternating, peak_above, graph, tables, row_err           # noqa: E402


def problem(name, G_csr, d, side, n_rows=None):
    """(Y, G, csr with weights, X, gX, transposed) of one half-sweep; n_rows: the first rows only."""
    T = tables(name, d)
    Y = T['item' if side == 'user' else 'user']
    rowptr, col = G_csr[side]
    if n_rows is not None:
        rowptr = rowptr[:n_rows + 1].contiguous()
        col = col[:int(rowptr[-1])].contiguous()
    g = torch.Generator(device='cuda').manual_seed(d + 1)
    val = (0.5 + 0.5 * torch.rand(col.numel(), device='cuda', generator=g))
    csr = (rowptr, col, val)
    G = als.gram(Y)
    X = alsgrad.als_solve_rows_target(Y, G, csr, ALPHA, REG, 'relaxed', route='fused', check_range=False)
    gX = torch.randn(X.shape, device='cuda', generator=g)
    tr = transpose_positives(rowptr, col, rowptr.numel() - 1, Y.shape[0])
    return Y, G, csr, X, gX, tr


def autograd_composed(Y, csr, gX):
    Yr, v = Y.clone().requires_grad_(True), csr[2].clone().requires_grad_(True)
    G = Yr.t() @ Yr
    X = alsgrad._solve_composed(Yr, G, csr[0], csr[1], v, ALPHA, REG, 'relaxed')
    return torch.autograd.grad((X * gX).sum(), (Yr, v))


def dval_err(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


def run_adjoint(name, G_csr, d, reps):
    lines = []
    for side in ('user', 'item'):
        Y, G, csr, X, gX, tr = problem(name, G_csr, d, side)
        deg = (csr[0][1:] - csr[0][:-1]).long()
        cdeg = (tr[0][1:] - tr[0][:-1]).long()
        out = dict(leg='adjoint', shape=name, side=side, dim=d, rows=int(deg.numel()), other_rows=int(Y.shape[0]), nnz=int(csr[1].numel()),
                   longest_row=int(deg.max()), longest_column=int(cdeg.max()))
        fns = {'kernel': lambda: alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, check_range=False),
               'composed': lambda: alsgrad.als_adjoint_composed(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr),
               'autograd_forward_backward': lambda: autograd_composed(Y, csr, gX),
               'composed_forward': lambda: alsgrad.als_solve_rows_target(Y, G, csr, ALPHA, REG, 'relaxed', route='composed'),
               'kernel_forward': lambda: alsgrad.als_solve_rows_target(Y, G, csr, ALPHA, REG, 'relaxed', route='fused', check_range=False)}
        t = alternating(fns, reps)
        out['time'] = t
        out['speedup_over_composed_median'] = t['composed']['median_s'] / t['kernel']['median_s']
        out['speedup_over_autograd_median'] = t['autograd_forward_backward']['median_s'] / (t['kernel']['median_s'] + t['kernel_forward']['median_s'])
        out['adjoint_over_forward_kernel'] = t['kernel']['median_s'] / t['kernel_forward']['median_s']
        out['kernel_peak_bytes'] = peak_above(fns['kernel'])
        out['composed_peak_bytes'] = peak_above(fns['composed'])
        out['autograd_peak_bytes'] = peak_above(fns['autograd_forward_backward'])
        csr64 = (csr[0], csr[1], csr[2].double())
        want = alsgrad.als_adjoint_composed(Y.double(), G, csr64, X.double(), gX.double(), ALPHA, REG, 'relaxed', transposed=tr)
        for k in ('kernel', 'composed'):
            got = fns[k]()
            out[k + '_dY_row_err'], out[k + '_dval_err'] = row_err(got[0], want[0]), dval_err(got[1], want[1])
        lines.append(out)
    return lines


def run_crossover(name, G_csr, d, reps):
    out = dict(leg='crossover', shape=name, side='user', dim=d, by_rows={})
    total = G_csr['user'][0].numel() - 1
    for n in (1, 8, 64, 512, 4096, total):
        Y, G, csr, X, gX, tr = problem(name, G_csr, d, 'user', n)
        t = alternating({'kernel': lambda: alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, check_range=False),
                         'composed': lambda: alsgrad.als_adjoint_composed(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr)}, reps)
        out['by_rows'][str(n)] = dict(kernel_median_s=t['kernel']['median_s'], composed_median_s=t['composed']['median_s'],
                                      speedup_median=t['composed']['median_s'] / t['kernel']['median_s'])
    ahead = [int(n) for n, v in out['by_rows'].items() if v['speedup_median'] >= 1.0]
    out['kernel_not_behind_from_rows'] = min(ahead) if ahead and all(out['by_rows'][str(m)]['speedup_median'] >= 1.0 for m in
                                                                      (1, 8, 64, 512, 4096, total) if m >= min(ahead)) else None
    return out


def run_colsplit(name, G_csr, d, reps):
    Y, G, csr, X, gX, tr = problem(name, G_csr, d, 'user')
    cdeg = (tr[0][1:] - tr[0][:-1]).long()
    out = dict(leg='colsplit', shape=name, side='user', dim=d, longest_column=int(cdeg.max()), mean_column=float(cdeg.double().mean()),
               default_col_split_len=alsgrad.default_col_split_len(), by_col_split_len={})
    base = alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, check_range=False)[0]
    for s in (128, 512, 1024, 4096, 2 ** 31 - 1):
        fn = lambda: alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, col_split_len=s, check_range=False)
        t = alternating({'k': fn}, reps)['k']
        t.update(split_columns=int((cdeg > s).sum()), max_abs_diff_to_default=float((fn()[0] - base).abs().max()))
        out['by_col_split_len'][str(s)] = t
    return out


def run_forward(name, G_csr, d, reps):
    lines = []
    for side in ('user', 'item'):
        Y, G, csr, X, gX, tr = problem(name, G_csr, d, side)
        t = alternating({'adjoint': lambda: alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, check_range=False),
                         'forward': lambda: als.als_solve_rows_kernel(Y, G, csr, ALPHA, REG, check_range=False)}, reps)
        lines.append(dict(leg='forward', shape=name, side=side, dim=d, rows=int(X.shape[0]), nnz=int(csr[1].numel()), time=t,
                          adjoint_over_forward_median=t['adjoint']['median_s'] / t['forward']['median_s'],
                          adjoint_peak_bytes=peak_above(lambda: alsgrad.als_adjoint_kernel(Y, G, csr, X, gX, ALPHA, REG, 'relaxed', transposed=tr, check_range=False)),
                          composed='not timed: the composed route does not hold this shape in a time worth measuring'))
    return lines


def run_revadv(name, d, reps):
    from arlib_amd.attack.Gray.RevAdv import RevAdv
    from arlib_amd.util import synthetic
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.tool import seedSet
    S = SHAPES[name]
    p = np.asarray(synthetic.syn_v1_pairs_native(S['U'], S['I'], S['deg'], 2018))
    one = (p[:, 0], p[:, 1], np.ones(len(p)))
    data = DataLoader.from_arrays(one, None, (p[:1, 0], p[:1, 1], np.ones(1)), dataName='syn')
    out = dict(leg='revadv', shape=name, dim=d, time={})
    W = None
    for route in ('fused', 'composed'):
        seedSet(2018)
        arg = SimpleNamespace(attackCategory='Gray', attackModelName='RevAdv', maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1,
                              outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5, emb_size=d, rev_route=route)
        atk = RevAdv(arg, data)
        W = atk.initial_block() if W is None else W
        out.update(fake_users=atk.fakeUserNum, items=atk.itemNum, budget=atk.maliciousFeedbackNum, sweeps=atk.rev_sweeps, unroll=atk.rev_unroll)
        fn = lambda: atk.hypergradient(W)
        try:
            out['time'][route] = alternating({route: fn}, reps)[route]
            out[route + '_peak_bytes'] = peak_above(fn)
        except torch.OutOfMemoryError as e:
            out['time'][route] = 'does not fit: %s' % str(e).split('.')[0]
    if all(isinstance(v, dict) for v in out['time'].values()):
        out['speedup_median'] = out['time']['composed']['median_s'] / out['time']['fused']['median_s']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='adjoint,crossover,colsplit,forward,revadv')
    ap.add_argument('--dims', default='64,128')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'alsgrad_bench.json'))
    a = ap.parse_args()
    assert torch.cuda.is_available(), 'alsgrad_bench needs a GPU'
    legs, dims = a.legs.split(','), [int(x) for x in a.dims.split(',')]
    lines = []

    def emit(x):
        for line in (x if isinstance(x, list) else [x]):
            lines.append(line)
            print(json.dumps(line), flush=True)
    t0 = time.time()
    if {'adjoint', 'crossover', 'colsplit'} & set(legs):
        g = graph('ml1m')
        for d in dims:
            if 'adjoint' in legs:
                emit(run_adjoint('ml1m', g, d, a.reps))
            if 'crossover' in legs:
                emit(run_crossover('ml1m', g, d, a.reps))
            if 'colsplit' in legs:
                emit(run_colsplit('ml1m', g, d, a.reps))
        del g
    if 'forward' in legs:
        g = graph('cfg2')
        for d in dims:
            emit(run_forward('cfg2', g, d, a.reps))
        del g
    if 'revadv' in legs:
        for d in dims:
            emit(run_revadv('ml1m', d, a.reps))
    out = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, wall_s=time.time() - t0, legs=lines)
    if os.path.exists(a.out) and set(legs) != {'adjoint', 'crossover', 'colsplit', 'forward', 'revadv'}:       # a partial run merges into the file
        old = json.load(open(a.out))
        keep = [l for l in old.get('legs', []) if l['leg'] not in legs]
        out['legs'] = keep + lines
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()

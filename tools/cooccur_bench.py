#!/usr/bin/env python3
"""The exact top-k co-occurrence neighbour op (arlib_amd/neighbours.py, csrc/arl_cooccur.hip) on both sides of two graphs: the user side
(neighbours of users) and the item side (neighbours of items: the transposed input), at ml-1M's shape (6 040 x 3 706, SYN-v1 pairs at ml-1M's
mean degree) and at cfg2's (SYN-v1, 1 M users x 100 K items).  Prints one JSON line and writes it to profiles/cooccur_bench.json.

    python tools/cooccur_bench.py [--reps 5] [--k 25] [--measure cosine] [--subset 32768] [--full-limit-s 60] [--host-rows 256] [--skip-cfg2] [--skip-host]

Per shape and side:
  plan_ms        the wrapper's preparation on the device (canonical rows, column-major index, launch order; host clock around a synchronise);
  kernel_ms      arl_cooccur_topk_i32 alone on that plan (device events; median, min, max of --reps after one warm-up), all rows as queries;
  call_ms        one neighbours.cooccur_topk(route='kernel') call: plan and kernel;
  increments, gincrements_per_s   the LDS counter increments the kernel issues (sum over the queries of the summed degrees of their columns,
                 counted from the input) and that count over kernel_ms;
  host_s         neighbours.cooccur_topk_host (scipy product, integer keys) on the same input, host clock, one run; and that the integers are equal;
  composed_ms    where n_rows^2 floats fit: fp32 X @ X.T on the device, float keys, torch.topk.  A timing yardstick only: its order among
                 tied and nearly tied keys is not the contract's.
At cfg2 the user side has 10^6 queries of 62 tiles each: the kernel is timed on --subset random queries first, and on all rows only when that
predicts at most --full-limit-s seconds; the host route is timed on --host-rows of those queries (the full product does not fit a host), and
there is no composed yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402
import scipy.sparse as sp                     # noqa: E402


def graph(U, I, mean_deg, seed=2018):
    from arlib_amd.util import synthetic
    p = synthetic.syn_v1_pairs_native(U, I, mean_deg, seed)
    X = sp.csr_matrix((np.ones(len(p), np.int64), (p[:, 0], p[:, 1])), shape=(U, I))
    X.sort_indices()
    return X


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return [statistics.median(times), min(times), max(times)]


def host_ms(fn, reps):
    import torch
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return [statistics.median(times), min(times), max(times)]


def side(X, a, full_host, name):
    """One side of one graph: X is n_rows x n_cols, its rows are the queries."""
    import torch
    from arlib_amd import _lib, neighbours, ops
    n, m = X.shape
    k, measure = a.k, a.measure
    rp = torch.from_numpy(X.indptr.astype(np.int64)).cuda()
    ci = torch.from_numpy(X.indices.astype(np.int32)).cuda()
    out = dict(side=name, n_rows=n, n_cols=m, nnz=int(X.nnz), k=k, measure=measure, tile_rows=neighbours.COOCCUR_DEFAULT_TILE_ROWS,
               tiles=-(-n // neighbours.COOCCUR_DEFAULT_TILE_ROWS), max_degree=int(np.diff(X.indptr).max()))

    def plan():
        crp, cci, r, deg = neighbours._canonical(rp, ci, n, m)
        colptr, irow, weight = neighbours._col_major(r, cci, n, m)
        return crp, cci, colptr, irow, weight, deg
    out['plan_ms'] = host_ms(plan, a.reps)
    crp, cci, colptr, irow, weight, deg = plan()
    L, P = _lib.lib(), ops._ptr

    def kernel(rows):
        Q = n if rows is None else rows.numel()
        wq = weight if rows is None else weight[rows.long()]
        order = torch.sort(wq, descending=True, stable=True).indices.to(torch.int32).contiguous()
        idx, cnt = torch.empty((Q, k), dtype=torch.int32, device='cuda'), torch.empty((Q, k), dtype=torch.int32, device='cuda')
        run = lambda: _lib.check(L.arl_cooccur_topk_i32(P(crp), P(cci), P(colptr), P(irow), n, m, P(rows), Q, k, neighbours.MEASURES[measure], out['max_degree'],
                                                        P(order), 0, P(idx), P(cnt), ops._stream()), 'arl_cooccur_topk_i32')
        return run, idx, cnt, float(wq.sum())
    rng = np.random.RandomState(1)
    rows_all = None
    if n > a.subset:
        sub = torch.from_numpy(np.sort(rng.choice(n, a.subset, replace=False)).astype(np.int32)).cuda()
        run, idx, cnt, inc = kernel(sub)
        t = events_ms(run, max(2, a.reps // 2))
        out.update(subset_queries=a.subset, subset_kernel_ms=t, subset_increments=inc, subset_gincrements_per_s=inc / t[0] / 1e6,
                   full_kernel_ms_predicted_from_subset=t[0] * n / a.subset)
        rows_all = sub
        if t[0] * n / a.subset > a.full_limit_s * 1e3:
            out['kernel_ms'] = None
            out['note'] = 'all rows not timed: the subset predicts more than --full-limit-s = %g s' % a.full_limit_s
    if 'kernel_ms' not in out:
        run, idx, cnt, inc = kernel(None)
        t = events_ms(run, a.reps)
        out.update(kernel_ms=t, increments=inc, gincrements_per_s=inc / t[0] / 1e6)
        out['call_ms'] = events_ms(lambda: neighbours.cooccur_topk(rp, ci, n, m, k, measure, route='kernel'), a.reps)
        rows_all = None
    # the host route: all rows where the product fits, --host-rows of the queries otherwise
    if full_host:
        hrows, got_i, got_c = None, idx.cpu().numpy(), cnt.cpu().numpy()
    else:
        pick = np.sort(rng.choice(n if rows_all is None else a.subset, a.host_rows, replace=False))
        hrows = pick if rows_all is None else rows_all.cpu().numpy()[pick].astype(np.int64)
        got_i, got_c = idx.cpu().numpy()[pick], cnt.cpu().numpy()[pick]
    if not a.skip_host:
        t0 = time.perf_counter()
        hi, hc, _ = neighbours.cooccur_topk_host(X, k, measure, hrows)
        out.update(host_s=time.perf_counter() - t0, host_queries=n if hrows is None else len(hrows),
                   host_equals_kernel=bool(np.array_equal(hi, got_i) and np.array_equal(hc, got_c)))
        out['host_ms_per_query'] = out['host_s'] * 1e3 / out['host_queries']
    if out.get('kernel_ms'):
        out['kernel_ms_per_query'] = out['kernel_ms'][0] / n
    # the composed route
    if n * n * 4 <= a.composed_limit_bytes:
        D = torch.zeros((n, m), dtype=torch.float32, device='cuda')
        D[torch.repeat_interleave(torch.arange(n, device='cuda'), deg), cci.long()] = 1.0
        dg = deg.float()

        def composed():
            C = D @ D.T
            if measure == 'cosine':
                S = C / torch.sqrt(dg[:, None] * dg[None, :]).clamp_min(1.0)
            elif measure == 'jaccard':
                S = C / (dg[:, None] + dg[None, :] - C).clamp_min(1.0)
            else:
                S = C.clone()
            S[C <= 0] = -1.0
            S.fill_diagonal_(-1.0)
            return torch.topk(S, min(k, n), dim=1)
        out['composed_ms'] = events_ms(composed, a.reps)
        cv, cidx = composed()
        mine = torch.where(idx >= 0, idx, torch.full_like(idx, -1)).long()
        theirs = torch.where(cv > 0, cidx, torch.full_like(cidx, -1))
        out['composed_lists_equal_to_kernel_share'] = float((mine[:, :theirs.shape[1]] == theirs).all(1).float().mean())
        del D
    else:
        out['composed_ms'] = None
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--k', type=int, default=25)
    ap.add_argument('--measure', default='cosine')
    ap.add_argument('--subset', type=int, default=32768)
    ap.add_argument('--full-limit-s', type=float, default=60.0)
    ap.add_argument('--host-rows', type=int, default=256)
    ap.add_argument('--composed-limit-bytes', type=int, default=4 << 30)
    ap.add_argument('--skip-cfg2', action='store_true')
    ap.add_argument('--skip-host', action='store_true', help='no host-route run (comparing two builds of the kernel)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cooccur_bench.json'))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('cooccur_bench: needs a GPU (a time taken anywhere else says nothing)')
    out = dict(device=torch.cuda.get_device_name(0), reps=a.reps, subset=a.subset, full_limit_s=a.full_limit_s, host_rows=a.host_rows, timing='device events around the call, one warm-up, median / min / max of reps; host_s one run on the host clock')
    X = graph(6040, 3706, 165.6)
    out['ml1m_shape'] = dict(users=6040, items=3706, nnz=int(X.nnz), sides=[side(X, a, True, 'user'), side(X.T.tocsr(), a, True, 'item')])
    if not a.skip_cfg2:
        X = graph(1_000_000, 100_000, 32.0)
        out['cfg2'] = dict(users=1_000_000, items=100_000, nnz=int(X.nnz), sides=[side(X, a, False, 'user'), side(X.T.tocsr(), a, False, 'item')])
    line = json.dumps(out)
    print(line)
    with open(a.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()

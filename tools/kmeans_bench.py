#!/usr/bin/env python3
"""NCL's prototype step on the device (arlib_amd/cluster.py) at cfg2's two table shapes with k = 2000.  Prints one JSON line.

    python tools/kmeans_bench.py [--users 1000000 --items 100000 --dim 64 --k 2000 --reps 7 --seeds 0 1 2] [--init k-means++] [--sklearn [--sklearn-limit 600]]

Per table (device events, two warm-up calls, the median of --reps windows, every window a batch of calls that fills about 50 ms):
`assign_kernels_ms`, the bias and assign kernels launched on buffers that exist already, and their share of the floor 2 N k d / 155 TFLOP/s
(exact-fp32 matrix rate); `assign_call_ms` and `update_call_ms`, one cluster.kmeans_assign / kmeans_update call as the loop makes it (output and
workspace allocations, for the update also the sort and prefix sums); and the whole cluster.kmeans call (host clock around a call that ends in
a host read).  `e_step_s` is the two tables together, what NCL.e_step costs with kmeans = 'device'.

--init k-means++ starts every cluster.kmeans call below from the device k-means++ start (arlib_amd/seeding.py) and adds, per table, `seeding_ms`:
one seeding.kmeanspp call with the draws made beforehand (k - 1 steps of a distance pass and a pick, all enqueued at once), against
`seeding_floor_ms`, the traffic of the k - 1 steps, (4 N d + 4 T N) bytes each, at 6.3 TB/s, and the launches (2 per step) that come on top.

--sklearn adds the yardstick on the ITEM table: the reference's run_kmeans (KMeans(n_clusters=k).fit(x), then predict(x)) in a child process that
never opens the GPU, once per seed, all under --sklearn-limit seconds; whatever finished before the limit is reported, and a run that did not
finish is reported as such with the limit as the lower bound of its time.  Quality: final inertia (float64, from the returned centroids and
labels, the same expression for both) per seed; the device's mean must not exceed sklearn's worst seed by more than sklearn's own spread
(max - min).  The device side walks n_iter = 20, 50, 100, 300 until that holds.  The child also times sklearn's own seeding,
sklearn.cluster.kmeans_plusplus(x, k), once per seed before the fits (`sklearn_kmeans_plusplus_s`).

The tables are synthetic (a trained table is not at hand at this size): --blobs latent groups with unequal sizes, centres 0.1 N(0, 1), rows
0.05 N(0, 1) around them -- the scale of trained embeddings, more groups than a tenth of k so that no cluster structure is handed to Lloyd for free."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402

MFMA_F32_TFLOPS = 155.0
HBM_TBS = 6.3                                 # achievable streaming rate
LADDER = (20, 50, 100, 300)


def table(n, d, blobs, seed):
    rng = np.random.default_rng(seed)
    centres = 0.1 * rng.standard_normal((blobs, d))
    group = np.floor(blobs * rng.random(n) ** 2).astype(np.int64)           # unequal group sizes
    return (centres[group] + 0.05 * rng.standard_normal((n, d))).astype(np.float32)


def inertia64(x, centres, labels):
    x, c = x.astype(np.float64), centres.astype(np.float64)
    return float(((x - c[labels]) ** 2).sum())


def sklearn_child(path, k, seeds):
    """The parent commit's NCL.run_kmeans on the host, one line of JSON per seed as soon as it is done."""
    from sklearn.cluster import KMeans, kmeans_plusplus
    x = np.load(path)
    for seed in seeds:
        np.random.seed(seed)
        t = time.perf_counter()
        kmeans_plusplus(x, k)
        print(json.dumps(dict(seed=seed, kmeans_plusplus_seconds=time.perf_counter() - t)), flush=True)
    for seed in seeds:
        np.random.seed(seed)
        t = time.perf_counter()
        km = KMeans(n_clusters=k).fit(x)
        labels = km.predict(x)
        s = time.perf_counter() - t
        print(json.dumps(dict(seed=seed, seconds=s, n_iter=int(km.n_iter_), inertia=inertia64(x, km.cluster_centers_, labels))), flush=True)


def device_events_ms(fn, reps, window_ms=50.0):
    """Milliseconds per call of fn: two warm-up calls, then `reps` event pairs, each around a batch of calls sized to fill `window_ms` (a single
    sub-millisecond call would measure the events and the launch path); returns (median, min, max, calls per batch)."""
    import torch

    def batch(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    inner = int(min(500, max(5, window_ms / max(batch(5), 1e-3))))
    times = [batch(inner) for _ in range(reps)]
    return statistics.median(times), min(times), max(times), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--k', type=int, default=2000)
    ap.add_argument('--blobs', type=int, default=300)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--seeds', type=int, nargs='+', default=[0, 1, 2])
    ap.add_argument('--init', choices=('random', 'k-means++'), default='random')
    ap.add_argument('--sklearn', action='store_true')
    ap.add_argument('--sklearn-limit', type=float, default=600.0)
    ap.add_argument('--sklearn-child', nargs=1, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.sklearn_child:
        return sklearn_child(a.sklearn_child[0], a.k, a.seeds)

    import torch
    from arlib_amd import cluster, seeding, _lib, ops
    if not torch.cuda.is_available():
        sys.exit('kmeans_bench: needs a GPU (a time taken anywhere else says nothing)')
    d, k = a.dim, a.k
    init = None if a.init == 'random' else a.init
    out = dict(dim=d, k=k, reps=a.reps, n_iter_default=cluster.kmeans.__defaults__[0], init=a.init)
    host = {'user': table(a.users, d, a.blobs, 1), 'item': table(a.items, d, a.blobs, 2)}
    e_step = 0.0
    for name, xh in host.items():
        X = torch.from_numpy(xh).cuda()
        N = X.shape[0]
        np.random.seed(0)
        C = X[torch.from_numpy(cluster.kmeans_init_indices(N, k)).cuda()]
        labels, score = cluster.kmeans_assign(X, C)
        bias = torch.empty(k, dtype=torch.float32, device='cuda')
        L, P = _lib.lib(), ops._ptr

        def kernels_only():                                                 # the bias and assign kernels on buffers that exist already
            _lib.check(L.arl_kmeans_assign_f32(P(X), N, P(C), k, d, P(bias), P(labels), P(score), ops._stream()), 'arl_kmeans_assign_f32')
        t_kernels = device_events_ms(kernels_only, a.reps)
        t_assign = device_events_ms(lambda: cluster.kmeans_assign(X, C), a.reps)
        t_update = device_events_ms(lambda: cluster.kmeans_update(X, labels, C, check_range=False), a.reps)
        floor_ms = 2.0 * N * k * d / (MFMA_F32_TFLOPS * 1e12) * 1e3
        whole = []
        for _ in range(3):
            np.random.seed(0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = cluster.kmeans(X, k, init=init)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t)
        e_step += statistics.median(whole)
        out[name] = dict(rows=N, assign_floor_ms=floor_ms,
                         assign_kernels_ms=t_kernels[0], assign_kernels_ms_min_max=t_kernels[1:3], assign_kernels_calls_per_window=t_kernels[3],
                         assign_kernels_share_of_floor=floor_ms / t_kernels[0], assign_kernels_tflops=2.0 * N * k * d / t_kernels[0] / 1e9,
                         assign_call_ms=t_assign[0], assign_call_ms_min_max=t_assign[1:3], assign_call_share_of_floor=floor_ms / t_assign[0],
                         update_call_ms=t_update[0], update_call_ms_min_max=t_update[1:3],
                         kmeans_s=statistics.median(whole), kmeans_updates=res[3], kmeans_assign_passes=len(res[2]))
        if init:
            np.random.seed(0)
            first, u = seeding.kmeanspp_draws(N, k)
            draws = (first, torch.from_numpy(u).cuda())
            t_seed = device_events_ms(lambda: seeding.kmeanspp(X, k, draws=draws), a.reps)
            step_bytes = 4.0 * N * d + 4.0 * u.shape[1] * N
            out[name].update(seeding_ms=t_seed[0], seeding_ms_min_max=t_seed[1:3], seeding_calls_per_window=t_seed[3], seeding_trials=u.shape[1],
                             seeding_launches=2 * k, seeding_floor_ms=(k - 1) * step_bytes / (HBM_TBS * 1e12) * 1e3,
                             seeding_step_us=t_seed[0] / (k - 1) * 1e3, seeding_tb_per_s=(k - 1) * step_bytes / t_seed[0] / 1e9)
        del X, C, labels, score, bias, res
    out['e_step_s'] = e_step

    if a.sklearn:
        xh = host['item']
        X = torch.from_numpy(xh).cuda()
        dev = {}
        for n_iter in LADDER:
            runs = []
            for seed in a.seeds:
                np.random.seed(seed)
                torch.cuda.synchronize()
                t = time.perf_counter()
                C, labels, _, done = cluster.kmeans(X, k, n_iter=n_iter, init=init)
                torch.cuda.synchronize()
                s = time.perf_counter() - t
                runs.append(dict(seed=seed, seconds=s, n_iter=done, inertia=inertia64(xh, C.cpu().numpy(), labels.cpu().numpy())))
            dev[n_iter] = runs
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, 'item_table.npy')
            np.save(path, xh)
            cmd = [sys.executable, os.path.abspath(__file__), '--k', str(k), '--seeds'] + [str(s) for s in a.seeds] + ['--sklearn-child', path]
            child = subprocess.Popen(cmd, stdout=subprocess.PIPE, text=True)
            try:
                text, finished = child.communicate(timeout=a.sklearn_limit)[0], True
            except subprocess.TimeoutExpired:
                child.kill()
                text, finished = child.communicate()[0], False
        lines = [json.loads(line) for line in text.splitlines() if line.startswith('{')]
        sk = [r for r in lines if 'inertia' in r]
        q = dict(sklearn_kmeans_plusplus_s=[r['kmeans_plusplus_seconds'] for r in lines if 'kmeans_plusplus_seconds' in r],
                 limit_s=a.sklearn_limit, all_seeds_finished=finished and len(sk) == len(a.seeds), sklearn=sk, device={str(n): r for n, r in dev.items()})
        if sk:
            q['time_ratio_sklearn_over_device'] = sk[0]['seconds'] / dev[LADDER[0]][0]['seconds']
        else:
            q['time_ratio_sklearn_over_device_at_least'] = a.sklearn_limit / dev[LADDER[0]][0]['seconds']
        if len(sk) >= 2:
            worst, spread = max(r['inertia'] for r in sk), max(r['inertia'] for r in sk) - min(r['inertia'] for r in sk)
            q['sklearn_worst_inertia'], q['sklearn_spread'] = worst, spread
            q['device_mean_inertia'] = {str(n): statistics.mean(r['inertia'] for r in runs) for n, runs in dev.items()}
            holds = [n for n in LADDER if q['device_mean_inertia'][str(n)] <= worst + spread]
            q['quality_holds_from_n_iter'] = holds[0] if holds else None
            q['device_over_sklearn_worst'] = {n: v / worst for n, v in q['device_mean_inertia'].items()}
        out['item_table_against_sklearn'] = q
    print(json.dumps(out))


if __name__ == '__main__':
    main()

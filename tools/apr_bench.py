#!/usr/bin/env python3
"""APR's adversarial-BPR term on the device (arlib_amd/advpair.py, csrc/arl_advpair.hip).  Prints one JSON line and writes it to --out.

    python tools/apr_bench.py [--reps 7 --out profiles/apr_bench.json --users 1000000 --items 100000]

Three measurements in one run, all by device events (two warm-up calls, the median of --reps windows, every window a batch of calls that
fills about 50 ms), the two sides of every comparison in alternating windows:

  function   util.loss.adv_bpr_loss forward + backward under autograd on [2048, d] rows with node ids as groups, d 64 and 128: the fused
             route (one kernel call over a packed copy) against the composed torch route on the same rows (`fused_ms`, `composed_ms`), and
             the kernel call alone on buffers that exist already (`kernel_ms`: its four launches).
  lightgcn   engine.step_apr against engine.step of the same engine on the cfg2 graph (SYN-v1, LightGCN, L 3, d 64, B 2048): `step_ms`,
             `step_apr_ms`, their difference, and `kernel_ms` of the compact-row call the step adds (groups given, plain store-add).
  gmf        the same pair on ml-1M's shape (6 040 users, 3 706 items, L 0: the dense form, uniform random batches).

Tables are xavier-uniform; batches are the sampler's (lightgcn) or uniform draws with n != p (function, gmf).  A time does not depend on the
values.  The robustness comparison (a GMF-trained against an APR-trained model under the same perturbation) is not part of this tool."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def alternating_ms(fns, reps, window_ms=50.0):
    """Milliseconds per call of every fn of the dict: two warm-up calls each, then `reps` rounds; a round times each fn once, an event pair
    around a batch of calls sized to fill `window_ms`.  Returns {name: (median, min, max, calls per batch)}."""
    import torch

    def batch(fn, n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / n
    inner = {}
    for name, fn in fns.items():
        fn(); fn()
        torch.cuda.synchronize()
        inner[name] = int(min(500, max(1, window_ms / max(batch(fn, 1), 1e-3))))
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            times[name].append(batch(fn, inner[name]))
    return {name: (statistics.median(t), min(t), max(t), inner[name]) for name, t in times.items()}


def entry(res, name):
    m = res[name]
    return {name + '_ms': m[0], name + '_ms_min_max': m[1:3], name + '_calls_per_window': m[3]}


def uniform_batch(torch, U, I, B, seed, dev):
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, U, (B,), generator=g).to(torch.int32)
    p = torch.randint(0, I, (B,), generator=g).to(torch.int32)
    n = (p + 1 + torch.randint(0, I - 1, (B,), generator=g).to(torch.int32)) % I
    return u.to(dev), p.to(dev), n.to(dev)


def xavier(torch, U, I, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.nn.init.xavier_uniform_(torch.empty(U, d), generator=g), torch.nn.init.xavier_uniform_(torch.empty(I, d), generator=g)], 0)


def function_leg(torch, d, B, reps, dev):
    from arlib_amd import ops, _lib
    from arlib_amd.util.loss import adv_bpr_loss, _adv_bpr_composed
    U, I = 943, 1682
    u, p, n = uniform_batch(torch, U, I, B, d, dev)
    rows = torch.cat([u, p + U, n + U])
    E = xavier(torch, U, I, d, d).to(dev)
    e = E[rows.long()].clone().requires_grad_(True)
    grp64 = rows.long()

    def fused():
        e.grad = None
        adv_bpr_loss(e[:B], e[B:2 * B], e[2 * B:], 0.5, groups=rows).backward()

    def composed():
        e.grad = None
        _adv_bpr_composed(e[:B], e[B:2 * B], e[2 * B:], 0.5, grp64).backward()
    packed = e.detach().contiguous()
    ar = torch.arange(B, dtype=torch.int32, device=dev)
    G, lo = torch.zeros_like(packed), torch.empty(2, device=dev)
    ws = torch.empty(_lib.lib().arl_bpr_adv_workspace_bytes(B, d) // 4, device=dev)

    def kernel():
        ops.bpr_adv_fwd_bwd(packed, B, ar, ar, ar + B, 0.5, groups=rows, G=G, workspace=ws, loss_out=lo, check_range=False, distinct_rows=True)
    res = alternating_ms({'fused': fused, 'composed': composed, 'kernel': kernel}, reps)
    out = dict(rows=B, dim=d, distinct_nodes=int(torch.unique(rows).numel()))
    for k in res:
        out.update(entry(res, k))
    out['composed_over_fused'] = res['composed'][0] / res['fused'][0]
    return out


def step_leg(torch, eng, batches, reps, what):
    from arlib_amd import ops, _lib
    k = {'step': 0, 'step_apr': 0}

    def step():
        b = batches[k['step'] % len(batches)]; k['step'] += 1
        eng.step(*b)

    def step_apr():
        b = batches[k['step_apr'] % len(batches)]; k['step_apr'] += 1
        eng.step_apr(*b, eps=0.5, adv_reg=1.0)
    fns = {'step': step, 'step_apr': step_apr}
    B, d = batches[0][0].numel(), eng.d
    u, p, n = batches[0]
    lo = torch.empty(2, device=eng.device)
    ws = torch.empty(_lib.lib().arl_bpr_adv_workspace_bytes(B, d) // 4, device=eng.device)
    if eng.L > 0:                             # the call the sparse form adds: compact rows, groups = node ids, plain store-add
        rows = torch.cat([u, p + eng.U, n + eng.U])
        packed, ar = eng.E0[rows.long()].contiguous(), torch.arange(B, dtype=torch.int32, device=eng.device)
        G = torch.zeros_like(packed)
        fns['kernel'] = lambda: ops.bpr_adv_fwd_bwd(packed, B, ar, ar, ar + B, 0.5, groups=rows, G=G, workspace=ws, loss_out=lo, check_range=False, distinct_rows=True)
    else:                                     # the call the dense form adds: real indices, ordered backward into the table-sized G
        G = torch.zeros_like(eng.E0)
        fns['kernel'] = lambda: ops.bpr_adv_fwd_bwd(eng.E0, eng.U, u, p, n, 0.5, G=G, workspace=ws, loss_out=lo, check_range=False)
    res = alternating_ms(fns, reps)
    out = dict(what=what, batch=B, dim=d, layers=eng.L)
    for name in res:
        out.update(entry(res, name))
    out['step_apr_minus_step_ms'] = res['step_apr'][0] - res['step'][0]
    out['step_apr_over_step'] = res['step_apr'][0] / res['step'][0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--mean-deg', type=float, default=32.0)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'apr_bench.json'))
    a = ap.parse_args()

    import numpy as np
    import torch
    from arlib_amd import ops, engine
    from arlib_amd.util import synthetic
    from arlib_amd.util.sampler import MTState
    if not torch.cuda.is_available():
        sys.exit('apr_bench: needs a GPU (a time taken anywhere else says nothing)')
    dev, B = 'cuda', a.batch
    out = dict(reps=a.reps, eps=0.5, adv_reg=1.0, function={}, robustness='not measured')
    for d in (64, 128):
        out['function'][str(d)] = function_leg(torch, d, B, a.reps, dev)

    # ---- LightGCN, L 3, on the cfg2 graph: bench.py's workload
    data = synthetic.syn_v1(a.users, a.items, a.mean_deg, a.seed)
    U, I, nnz = data.training_size()
    rowptr, col = data.adjacency_pattern()
    col_d = torch.from_numpy(col).to(dev)
    val, _ = ops.norm_adj_values(torch.from_numpy(rowptr.astype(np.int32)).to(dev), col_d, torch.ones(2 * nnz, dtype=torch.float32, device=dev), U + I)
    A = ops.CSRGraph(rowptr, col_d, val, dev, validate=True)
    mt = MTState.from_seed(a.seed)
    data.pair_sampler.shuffle(mt)
    nb = max(1, min(32, nnz // B))
    hb = np.empty((nb, 3, B), np.int32)
    for k in range(nb):
        data.pair_sampler.batch(mt, k * B, B, out=hb[k])
    batches = [tuple(torch.from_numpy(hb[k, j]).to(dev) for j in range(3)) for k in range(nb)]
    eng = engine.PropagationEngine(A, U, I, 64, 3, 1e-4, 0.005, dev, table=xavier(torch, U, I, 64, a.seed).to(dev))
    out['lightgcn'] = step_leg(torch, eng, batches, a.reps, 'SYN-v1 %d users x %d items, nnz %d, LightGCN L 3 d 64, sparse-batch form' % (U, I, nnz))
    del eng, A, val, col_d
    torch.cuda.empty_cache()

    # ---- GMF on ml-1M's shape: the dense form
    U, I = 6040, 3706
    eng = engine.PropagationEngine(None, U, I, 64, 0, 1e-4, 0.005, dev, table=xavier(torch, U, I, 64, a.seed).to(dev))
    batches = [uniform_batch(torch, U, I, B, 100 + k, dev) for k in range(32)]
    out['gmf'] = step_leg(torch, eng, batches, a.reps, 'ml-1M shape: %d users x %d items, GMF (L 0) d 64, dense form' % (U, I))

    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()

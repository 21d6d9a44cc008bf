"""SSL4Rec timings at cfg2 (1 M users + 100 K items, d = 64, B = 2048): the fused SSL4Rec step (engine.step_ssl4rec), the plain L = 2
engine.step on the same batch, and the contrastive term alone -- the dropout-view InfoNCE kernel (ops.ssl_dropout_nce) against the composed
nn.Dropout + ops.infonce_fwd_bwd x 2.  Also the step-for-step difference of the fused step against the autograd route.  Prints one JSON line.

    python tools/ssl4rec_bench.py [--reps 20]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arlib_amd import ops                                      # noqa: E402
from arlib_amd.engine import PropagationEngine                 # noqa: E402
from arlib_amd.util import synthetic                           # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        ev0.record(); fn(); ev1.record()
        torch.cuda.synchronize()
        ts.append(ev0.elapsed_time(ev1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    a = ap.parse_args()
    U, I, d, B = a.users, a.items, 64, 2048
    dev = torch.device('cuda', 0)
    data = synthetic.syn_v1(U, I, 32.0, 2018)
    nnz = data.training_size()[2]
    rowptr, col = data.adjacency_pattern()
    col_d = torch.from_numpy(col).to(dev)
    val, _ = ops.norm_adj_values(torch.from_numpy(rowptr.astype(np.int32)).to(dev), col_d, torch.ones(2 * nnz, device=dev), U + I)
    A = ops.CSRGraph(rowptr, col_d, val, dev)
    torch.manual_seed(2018)
    E0 = (torch.rand(U + I, d, device=dev) * 2 - 1) * 0.05
    g = torch.Generator().manual_seed(1)
    u = torch.randint(0, U, (B,), generator=g).to(torch.int32).to(dev)
    p = torch.randint(0, I, (B,), generator=g).to(torch.int32).to(dev)
    n = torch.randint(0, I, (B,), generator=g).to(torch.int32).to(dev)
    res = {'users': U, 'items': I, 'd': d, 'B': B}

    eng_plain = PropagationEngine(A, U, I, d, 2, 1e-4, 1e-3, dev, table=E0.clone())
    eng_ssl = PropagationEngine(A, U, I, d, 2, 1e-4, 1e-3, dev, table=E0.clone())
    res['plain_step_ms'] = timed(lambda: eng_plain.step(u, p, n), a.reps)
    res['ssl4rec_step_ms'] = timed(lambda: eng_ssl.step_ssl4rec(u, p, n), a.reps)
    res['ssl4rec_minus_plain_ms'] = res['ssl4rec_step_ms'] - res['plain_step_ms']

    Xu, Xp = eng_ssl.out_c[:B].clone(), eng_ssl.out_c[B:2 * B].clone()
    res['cl_kernel_ms'] = timed(lambda: ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=1, stream_id=2), a.reps)
    drop = torch.nn.Dropout(0.2)

    def composed():
        # the route without the kernel: four dropout draws, two InfoNCE calls, the chain rule through the dropout by hand
        out = []
        for X in (Xu, Xp):
            m1 = drop(torch.ones_like(X)); m2 = drop(torch.ones_like(X))
            loss, g1, g2 = ops.infonce_fwd_bwd((X * m1).contiguous(), (X * m2).contiguous(), 0.2)
            out.append((loss, g1 * m1 + g2 * m2))
        return out
    res['cl_composed_ms'] = timed(composed, a.reps)
    res['cl_speedup'] = res['cl_composed_ms'] / res['cl_kernel_ms']
    # 2 sides x (forward + dA product, logit recompute + dV product) = 8 n^2 d multiply-adds
    res['cl_gflop'] = 2 * 4 * 2.0 * B * B * d / 1e9
    res['cl_tflops'] = res['cl_gflop'] / res['cl_kernel_ms']                 # GFLOP per ms = TFLOP/s
    print(json.dumps(res))


if __name__ == '__main__':
    main()

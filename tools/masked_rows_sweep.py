"""Sweep of the two batch-row hops of the LightGCN step at the benchmark's shapes (SYN-v1 1M x 100K, d = 64, B = 2048):
  rows    ops.spmm_rows with the starting piece length P in --pieces (the library doubles it when the workspace is too small)
  masked  ops.spmm_flagged on the blocked plan against the CSR row-per-group kernel
Times are HIP-event averages over --iters calls after --warmup.  Prints one JSON line."""
import argparse
import json
import os
import sys
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000); ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--mean-deg', type=float, default=32.0); ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--batch', type=int, default=2048); ap.add_argument('--nsplit', type=int, default=32)
    ap.add_argument('--pieces', default='64,128,256,512,1024,2048,4096'); ap.add_argument('--warmup', type=int, default=5); ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--seed', type=int, default=2018)
    args = ap.parse_args()
    from arlib_amd import ops
    from arlib_amd.util import synthetic
    from arlib_amd.util.sampler import MTState
    dev = 'cuda:0'
    data = synthetic.syn_v1(args.users, args.items, args.mean_deg, args.seed)
    U, I, nnz = data.training_size()
    N, d, B = U + I, args.emb, args.batch
    rowptr, col = data.adjacency_pattern()
    col_d = torch.from_numpy(col).to(dev)
    val, _ = ops.norm_adj_values(torch.from_numpy(rowptr.astype(np.int32)).to(dev), col_d, torch.ones(2 * nnz, dtype=torch.float32, device=dev), N)
    A = ops.CSRGraph(rowptr, col_d, val, dev)
    Ab = ops.CSRGraph(rowptr, col_d, val, dev)
    ops.auto_blocked(Ab, d, split=U, force=True)
    mt = MTState.from_seed(args.seed)
    data.pair_sampler.shuffle(mt)
    b = torch.from_numpy(data.pair_sampler.batch(mt, 0, B)).to(dev)
    rows = torch.cat([b[0], b[1] + U, b[2] + U]).to(torch.int32).contiguous()
    torch.manual_seed(args.seed)
    X = torch.randn(N, d, device=dev)
    out = {'n_rows': int(rows.numel()), 'edges': int((torch.from_numpy(np.diff(rowptr)).to(dev)[rows.long()]).sum()), 'lib': ops._lib.LIB_PATH, 'rows_ms': {}, 'rows_plan': {}}
    ws = torch.empty(rows.numel() * args.nsplit * d, dtype=torch.float32, device=dev)
    o = torch.empty(rows.numel(), d, device=dev)
    for P in [int(x) for x in args.pieces.split(',')]:
        out['rows_ms'][P] = timed(lambda: ops.spmm_rows(A, X, rows, (X, X, X), 0.25, nsplit=args.nsplit, out=o, workspace=ws, check_range=False, piece_edges=P), args.warmup, args.iters)
        out['rows_plan'][P] = list(ops.spmm_rows_plan(ws, rows.numel(), args.nsplit, d)[:2])
    G = torch.zeros(N, d, device=dev); G[rows.long()] = torch.randn(rows.numel(), d, device=dev)
    bits = torch.zeros((N + 31) // 32, dtype=torch.int32, device=dev)
    ops.mark_bits_(bits, rows, True, N)
    flags = torch.zeros(N, dtype=torch.uint8, device=dev); flags[rows.long()] = 1
    Y = torch.empty(N, d, device=dev)
    out['masked_ms'] = {'blocked': timed(lambda: ops.spmm_flagged(Ab, G, bits, 1.0, 1.0, G, flags, out=Y), args.warmup, args.iters),
                        'csr': timed(lambda: ops.spmm_flagged(A, G, bits, 1.0, 1.0, G, flags, out=Y), args.warmup, args.iters)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()

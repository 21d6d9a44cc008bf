#!/usr/bin/env python3
"""The target-rank op: the streaming kernel (ops.target_rank_kernel) against the composed torch route (panels of 128 user rows), with peak memory, at
ml-1M's shape (6 040 x 3 706, d 64, T 5) and at cfg2's (1 M x 100 K, d 64, T 5, 16, 32 and 64), with and without a mask of 32 M entries (1 M at ml-1M's shape)
drawn uniformly, rows sorted and distinct.  Prints one JSON line per leg and writes them all to profiles/rank_bench.json.

    python tools/rank_bench.py [--shape cfg2|ml1m|both --dim 64 --reps 3 --composed-rows 20000 --out profiles/rank_bench.json]

The composed route at cfg2's size is 7 813 panels of 128 x 100 000 scores with T compare-and-count passes each, so it is timed on the first
--composed-rows user rows and scaled linearly in U (its cost per panel does not depend on U); the JSON says so.  The floor is the score product alone,
2 U I d flops at the fp32 matrix peak."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                  # noqa: E402
from arlib_amd import ops                     # noqa: E402

SHAPES = {'ml1m': (6040, 3706, 1_000_209, (5,)), 'cfg2': (1_000_000, 100_000, 32_000_000, (5, 16, 32, 64))}
PEAK_TFLOPS = 157.3                           # fp32 matrix peak of the MI355X


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def uniform_mask(U, I, nnz, g, dev='cuda'):
    """CSR with nnz // U (+ 1) entries per row, each row sorted and distinct: a row's entries fall into equal strata of the item range, one per stratum."""
    deg = torch.full((U,), nnz // U, dtype=torch.int64, device=dev)
    deg[:nnz % U] += 1
    rowptr = torch.zeros(U + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = deg.cumsum(0).to(torch.int32)
    rows = torch.repeat_interleave(torch.arange(U, device=dev), deg, output_size=nnz)
    pos = torch.arange(nnz, device=dev) - rowptr[:-1].long()[rows]
    width = I // deg[rows]
    off = torch.minimum((torch.rand(nnz, device=dev, generator=g) * width).long(), width - 1)
    return rowptr, (pos * width + off).to(torch.int32)


def run(name, d, reps, composed_rows):
    U, I, nnz, Ts = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(0)
    Pu, Pi = torch.randn(U, d, device='cuda', generator=g) * 0.1, torch.randn(I, d, device='cuda', generator=g) * 0.1
    mask = uniform_mask(U, I, nnz, g)
    Uc = min(U, composed_rows)
    sub_mask = (mask[0][:Uc + 1].contiguous(), mask[1][:int(mask[0][Uc])].contiguous())
    Pus = Pu[:Uc].contiguous()
    legs = []
    for T in Ts:
        targets = torch.randperm(I, device='cuda', generator=g)[:T].to(torch.int32)
        for masked in (False, True):
            m, ms = (mask, sub_mask) if masked else (None, None)
            out = dict(shape=name, users=U, items=I, dim=d, targets=T, mask_nnz=nnz if masked else 0)
            kern = lambda: ops.target_rank_kernel(Pu, Pi, targets, m, check_range=False)
            comp = lambda: ops.target_rank_composed(Pus, Pi, targets, ms, check_range=False)
            out['kernel_s'] = timed(kern, reps)
            out['kernel_peak_bytes'] = peak_bytes(kern)
            out['floor_s'] = 2.0 * U * I * d / (PEAK_TFLOPS * 1e12)
            out['kernel_tflops'] = 2.0 * U * I * d / out['kernel_s'] / 1e12
            out['kernel_share_of_floor'] = out['floor_s'] / out['kernel_s']
            out['composed_rows_timed'] = Uc
            out['composed_s_scaled'] = timed(comp, 1 if name == 'cfg2' else reps) * U / Uc
            out['composed_peak_bytes'] = peak_bytes(comp)
            out['speedup'] = out['composed_s_scaled'] / out['kernel_s']
            rk, rc = kern()[0][:Uc], comp()[0]
            out['pairs_where_the_routes_differ'] = int((rk != rc).sum())          # near-ties inside the fp32 rounding bound (tests/rank_restatement.py)
            out['pairs_compared'] = rk.numel()
            print(json.dumps(out), flush=True)
            legs.append(out)
    return legs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('cfg2', 'ml1m', 'both'), default='both')
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--composed-rows', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'rank_bench.json'))
    a = ap.parse_args()
    legs = []
    for name in (('ml1m', 'cfg2') if a.shape == 'both' else (a.shape,)):
        legs += run(name, a.dim, a.reps, a.composed_rows)
    with open(a.out, 'w') as fh:
        json.dump({'tool': 'tools/rank_bench.py', 'device': torch.cuda.get_device_name(0), 'best_of': a.reps, 'legs': legs}, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

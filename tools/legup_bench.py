#!/usr/bin/env python3
"""LegUP's ranking loss: the streaming kernel (ops.colsoftmax_target_loss) against the composed torch route (panels of 128 user rows) at cfg2's
shape, and one inner iteration of the G phase (inject, sample, retrain, L_RS) end to end on ml-100k.  Prints one JSON line.

    python tools/legup_bench.py [--users 1000000 --items 100000 --dim 64 --targets 5 --reps 3 --composed-users 20000 --no-iteration]

The composed route at full size takes minutes (7 813 panels of 128 x 100 000 scores, two passes), so it is timed on the first --composed-users rows
and scaled linearly in U (its cost per panel does not depend on U)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                  # noqa: E402
from arlib_amd import ops                     # noqa: E402


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


def iteration_seconds():
    """One inner iteration of the G phase on ml-100k (the fixture tests/golden/ml100k_data.npz), recommender maxEpoch = 1."""
    from types import SimpleNamespace
    import numpy as np
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.attack.Gray.LegUP import LegUP, default_recommender_args
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', 'ml100k_data.npz'))
    data = DataLoader.from_arrays((g['train_u'], g['train_i'], g['train_r']), (g['val_u'], g['val_i'], g['val_r']), (g['test_u'], g['test_i'], g['test_r']),
                                  dataName='ml-100k')
    arg = SimpleNamespace(attackCategory='Gray', attackModelName='LegUP', times=1, poisonDatasetOutPath='data/poison/', poisondataSaveFlag=False,
                          maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, gradMaxLimitation=1, gradNumLimitation=60,
                          gradIterationNum=10, attackTargetChooseWay='unpopular', targetSize=5)
    atk = LegUP(arg, data, rec_args=default_recommender_args(maxEpoch=1))
    atk.selectItem = list(range(atk.itemNum // 5)) + atk.targetItem
    atk.Tepoch = 1
    atk._g_step()
    torch.cuda.synchronize()
    t = time.perf_counter()
    atk._g_step()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--targets', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--composed-users', type=int, default=20000)
    ap.add_argument('--no-iteration', action='store_true')
    a = ap.parse_args()
    U, I, d, T = a.users, a.items, a.dim, a.targets
    g = torch.Generator(device='cuda').manual_seed(0)
    Pu, Pi = torch.randn(U, d, device='cuda', generator=g) * 0.1, torch.randn(I, d, device='cuda', generator=g) * 0.1
    cols = list(range(I // 5, I // 5 + T))
    out = dict(users=U, items=I, dim=d, targets=T)
    out['kernel_loss_s'] = timed(lambda: ops.colsoftmax_target_loss(Pu, Pi, cols), a.reps)
    out['kernel_loss_grad_s'] = timed(lambda: ops.colsoftmax_target_loss(Pu, Pi, cols, want_grad=True), a.reps)
    flop = 2.0 * U * I * d
    out['kernel_loss_tflops'] = flop / out['kernel_loss_s'] / 1e12                     # one score pass
    out['kernel_loss_grad_tflops'] = 5 * flop / out['kernel_loss_grad_s'] / 1e12       # three score passes, two weighted row sums
    Uc = min(U, a.composed_users)
    sub = Pu[:Uc].contiguous()
    out['composed_users_timed'] = Uc
    out['composed_loss_s_scaled'] = timed(lambda: ops.colsoftmax_target_loss_composed(sub, Pi, cols), 1) * U / Uc
    out['composed_loss_grad_s_scaled'] = timed(lambda: ops.colsoftmax_target_loss_composed(sub, Pi, cols, want_grad=True), 1) * U / Uc
    if not a.no_iteration:
        out['g_inner_iteration_s'] = iteration_seconds()
    print(json.dumps(out))


if __name__ == '__main__':
    main()

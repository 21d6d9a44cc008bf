#!/usr/bin/env python3
"""The uniformity term on the device (arlib_amd/pairloss.py) at d 64: the batch (n = 2 048), cfg2's item table (n = 100 000) and its user table
(n = 1 000 000).  Prints one JSON line and writes it to --out.

    python tools/pairloss_bench.py [--dim 64 --rows 2048 32768 100000 1000000 --reps 7 --out profiles/pairloss_bench.json]

Per size (device events, two warm-up calls, the median of --reps windows, every window a batch of calls that fills about 50 ms; one call per
window from 100 ms per call on): `kernels_ms`, arl_uniformity_fwd_bwd_f32 on buffers that exist already (every launch of the call: normalise, q,
pairs, row sums, total, finish, normalise backward), and its share of the floor 4 n^2 d / 155 TFLOP/s (two exact-fp32 products per ordered pair:
the scores and sum_j e_ij y_j; the both-orders sweep is counted as the work, so skipping a triangle would show as a share above 1);
`forward_ms` likewise without the gradient (floor 2 n^2 d); up to 200 000 rows also `call_ms`, one pairloss.uniformity call with its allocations,
and `function_ms`, util.loss.uniformity_loss forward + backward under autograd.  `composed_ms` is the reference's expression (F.normalize, torch.pdist, pow, mul,
exp, mean, log) forward + backward on the same rows, taken while the n (n - 1) / 2 distances stay below 2^31 elements (n <= 65 536: pdist's
result is indexed in int32 on the device) and its peak memory fits; beyond that the route does not exist and the entry says so.

Rows are 0.05 N(0, 1) (the scale of trained embeddings); the time does not depend on the values."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_F32_TFLOPS = 155.0
PDIST_MAX_ROWS = 65536                        # n (n - 1) / 2 < 2^31


def device_events_ms(fn, reps, window_ms=50.0):
    """Milliseconds per call of fn: two warm-up calls, then `reps` event pairs, each around a batch of calls sized to fill `window_ms`;
    returns (median, min, max, calls per batch)."""
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
    inner = int(min(500, max(1, window_ms / max(batch(1), 1e-3))))
    times = [batch(inner) for _ in range(reps)]
    return statistics.median(times), min(times), max(times), inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--rows', type=int, nargs='+', default=[2048, 32768, 100_000, 1_000_000])
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pairloss_bench.json'))
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    from arlib_amd import pairloss, _lib, ops
    from arlib_amd.util.loss import uniformity_loss
    if not torch.cuda.is_available():
        sys.exit('pairloss_bench: needs a GPU (a time taken anywhere else says nothing)')
    d = a.dim
    L, P = _lib.lib(), ops._ptr
    out = dict(dim=d, t=2, reps=a.reps, mfma_f32_tflops=MFMA_F32_TFLOPS, sizes={})
    for n in a.rows:
        big = n > 200_000                                # seconds per call: the kernels alone, fewer windows
        reps = 2 if big else a.reps
        g = torch.Generator().manual_seed(n)
        x = (0.05 * torch.randn(n, d, generator=g)).cuda()
        ws = torch.empty(L.arl_uniformity_workspace_bytes(n, d), dtype=torch.uint8, device='cuda')
        loss, dX = torch.empty(1, device='cuda'), torch.empty_like(x)

        def kernels(grad=True):
            _lib.check(L.arl_uniformity_fwd_bwd_f32(P(x), n, d, 2.0, 1.0, P(loss), P(dX) if grad else None, P(ws), ops._stream()), 'arl_uniformity_fwd_bwd_f32')
        t_k = device_events_ms(kernels, reps)
        t_f = device_events_ms(lambda: kernels(False), reps)
        xr = x.clone().requires_grad_(True)

        def function():
            xr.grad = None
            uniformity_loss(xr).backward()
        floor_ms = 4.0 * n * n * d / (MFMA_F32_TFLOPS * 1e12) * 1e3
        e = dict(rows=n, splits=pairloss.uniformity_splits(n), workspace_mib=ws.numel() / 2 ** 20, floor_ms=floor_ms,
                 kernels_ms=t_k[0], kernels_ms_min_max=t_k[1:3], kernels_calls_per_window=t_k[3], kernels_share_of_floor=floor_ms / t_k[0],
                 kernels_tflops=4.0 * n * n * d / t_k[0] / 1e9,
                 forward_ms=t_f[0], forward_ms_min_max=t_f[1:3], forward_share_of_floor=0.5 * floor_ms / t_f[0],
                 loss=float(loss))
        del ws, dX
        if not big:
            t_c = device_events_ms(lambda: pairloss.uniformity(x), reps)
            t_fn = device_events_ms(function, reps)
            e.update(call_ms=t_c[0], call_ms_min_max=t_c[1:3], function_ms=t_fn[0], function_ms_min_max=t_fn[1:3])
        if n <= PDIST_MAX_ROWS:
            def composed():
                xr.grad = None
                torch.pdist(F.normalize(xr, dim=-1), p=2).pow(2).mul(-2).exp().mean().log().backward()
            try:
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
                t_p = device_events_ms(composed, reps)
                e.update(composed_ms=t_p[0], composed_ms_min_max=t_p[1:3], composed_peak_mib=(torch.cuda.max_memory_allocated() - before) / 2 ** 20,
                         composed_over_function=t_p[0] / t_fn[0], composed_over_kernels=t_p[0] / t_k[0])
            except torch.cuda.OutOfMemoryError:
                e['composed'] = 'out of memory'
        else:
            e['composed'] = 'no route: %.3g distances, past the 2^31 elements pdist indexes (%.1f GB each in fp32)' % (n * (n - 1) / 2, n * (n - 1) / 2 * 4 / 1e9)
        out['sizes'][str(n)] = e
        del x, xr
        torch.cuda.empty_cache()
    text = json.dumps(out)
    print(text)
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()

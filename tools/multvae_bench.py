#!/usr/bin/env python3
"""The multinomial likelihood (csrc/arl_multinomial.hip) against the composed torch route, and the shares of one Mult-VAE training step, at ml-1M's
shape (B 500 users x I 3 706 items, d 64) and at cfg2's (B 2 048 and B 500 x I 100 000, d 64).  Prints one JSON line per leg and writes them all to
profiles/multvae_bench.json.

    python tools/multvae_bench.py [--shape ml1m|cfg2|cfg2_b500|all --reps 7 --inner 0 --out profiles/multvae_bench.json]

Legs per shape:
  op     forward + backward (nll, lse, dq, dE) and forward alone, kernel and composed on the same inputs.  A timed window is `inner` calls between two
         device synchronises on the host clock (inner is chosen so that a window lasts about 0.2 s unless given); the two routes' windows ALTERNATE,
         --reps of each after a warm-up, and the minimum, the median and the largest window are reported per call.  Peak device memory above the inputs.
         The kernel's share of the exact-fp32 MFMA floor: its passes cost 10 B I d flop (five score-sized products: the scores three times, and the
         two weighted row sums) against the fp32 matrix peak.  Both routes' errors against float64 on the first 128 rows.
  step   one training step of MultVAE on a SYN-v1 graph of the shape's item count on each route: the whole step, and its parts timed on their own
         between synchronises: the op (forward + backward on the step's own z and W_dec), the optimizer (torch Adam on the dense weights) and the
         encoder with everything else (batch CSR, its transpose, the two sparse products, KL, autograd bookkeeping) as the remainder.
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
import scipy.sparse as sp                     # noqa: E402
import torch                                  # noqa: E402
from arlib_amd import multinomial as mn       # noqa: E402

SHAPES = {'ml1m': dict(B=500, I=3706, U=6040, deg=165.6), 'cfg2': dict(B=2048, I=100_000, U=20_000, deg=32.0),
          'cfg2_b500': dict(B=500, I=100_000, U=20_000, deg=32.0)}
PEAK_TFLOPS = 157.3                           # fp32 matrix peak of the MI355X


def window(fn, inner):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / inner


def alternating(fns, reps, inner=0):
    """{name: (min, median, max) seconds per call}: every route warmed up, then --reps rounds in which each route gets one window."""
    inn = {}
    for name, fn in fns.items():
        fn(); fn()
        inn[name] = inner or max(1, min(200, int(0.2 / max(window(fn, 1), 1e-5))))
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


def rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def float64_op(q, E, P, g):
    q, E = q.double().cpu().requires_grad_(), E.double().cpu().requires_grad_()
    z = q @ E.t()
    A = torch.zeros_like(z)
    rp = P[0].cpu().long()
    A[torch.repeat_interleave(torch.arange(q.shape[0]), rp[1:] - rp[:-1]), P[1].cpu().long()] = 1.0
    lse = torch.logsumexp(z, 1)
    nll = A.sum(1) * lse - (A * z).sum(1)
    (g.double().cpu() * nll).sum().backward()
    return nll.detach(), lse.detach(), q.grad, E.grad


def problem(B, I, d, deg, g):
    q, E = torch.randn(B, d, device='cuda', generator=g), torch.randn(I, d, device='cuda', generator=g) / d ** 0.5
    n = torch.clamp((deg * torch.exp(torch.randn(B, device='cuda', generator=g) - 0.5)).long(), 1, I)       # log-normal profile sizes of mean deg
    rowptr = torch.zeros(B + 1, dtype=torch.int32, device='cuda')
    rowptr[1:] = torch.cumsum(n, 0)
    cols = [torch.randperm(I, device='cuda', generator=g)[:int(k)].sort()[0] for k in n.tolist()]
    return q, E, (rowptr, torch.cat(cols).to(torch.int32)), torch.full((B,), 1.0 / B, device='cuda')


def run_op(name, d, reps, inner):
    S = SHAPES[name]
    B, I = S['B'], S['I']
    g = torch.Generator(device='cuda').manual_seed(0)
    q, E, P, up = problem(B, I, d, S['deg'], g)
    pos_t = mn.transpose_positives(P[0], P[1], B, I)
    out = dict(leg='op', shape=name, batch_users=B, items=I, dim=d, positives=int(P[1].numel()))
    kern = lambda: mn.multinomial_softmax_kernel(q, E, P, up, want_grad=True, pos_t=pos_t, check_range=False)
    comp = lambda: mn.multinomial_softmax_composed(q, E, P, up, want_grad=True)
    t = alternating({'kernel': kern, 'composed': comp}, reps, inner)
    out['fwd_bwd'] = t
    out['fwd'] = alternating({'kernel': lambda: mn.multinomial_softmax_kernel(q, E, P, check_range=False), 'composed': lambda: mn.multinomial_softmax_composed(q, E, P)},
                             reps, inner)
    out['speedup_fwd_bwd_median'] = t['composed']['median_s'] / t['kernel']['median_s']
    out['speedup_fwd_median'] = out['fwd']['composed']['median_s'] / out['fwd']['kernel']['median_s']
    out['kernel_peak_bytes'], out['composed_peak_bytes'] = peak_above(kern), peak_above(comp)
    out['one_fp32_B_x_I_matrix_bytes'] = 4 * B * I
    out['kernel_flop'] = 10.0 * B * I * d
    out['mfma_floor_s'] = out['kernel_flop'] / (PEAK_TFLOPS * 1e12)
    out['kernel_share_of_fp32_mfma_floor'] = out['mfma_floor_s'] / t['kernel']['median_s']
    n = min(B, 128)
    sub = (q[:n].contiguous(), E, (P[0][:n + 1].contiguous(), P[1][:int(P[0][n])].contiguous()), up[:n].contiguous())
    want = float64_op(*sub)
    k, c = mn.multinomial_softmax_kernel(*sub, want_grad=True), mn.multinomial_softmax_composed(*sub, want_grad=True)
    out['error_rows'] = n
    for nm, a, b, w in zip(('nll', 'lse', 'dq', 'dE'), k, c, want):
        out['kernel_err_' + nm], out['composed_err_' + nm] = rel(a, w), rel(b, w)
    return out


def run_step(name, d, reps, inner):
    from arlib_amd.util import synthetic
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender import MultVAE
    S = SHAPES[name]
    U, I, B = S['U'], S['I'], S['B']
    p = np.asarray(synthetic.syn_v1_pairs_native(U, I, S['deg'], 2018))
    data = SimpleNamespace(user_num=U, item_num=I, interaction_mat=sp.csr_matrix((np.ones(len(p), np.float32), (p[:, 0], p[:, 1])), shape=(U, I)))
    out = dict(leg='step', shape=name, users=U, items=I, train_pairs=int(len(p)), batch_users=B, dim=d)
    for route in ('fused', 'composed'):
        seedSet(2018)
        with contextlib.redirect_stdout(io.StringIO()):
            rec = MultVAE(SimpleNamespace(dataset='syn-' + name, model_name='MultVAE', maxEpoch=1, batch_size=2048, emb_size=d, n_layers=0, reg=1e-4, lRate=1e-3,
                                          seed=2018, topK='50', vae_batch_users=B, vae_route=route), data)
        m = rec.model.cuda()
        opt = torch.optim.Adam(rec._params(), lr=1e-3)
        rows = torch.randperm(U)[:B].to('cuda')
        keep, eps = rec.draw(rows)
        keep, eps = keep.to('cuda'), eps.to('cuda')
        rowptr, col, _ = m.batch_csr(rows)
        P = (rowptr.to(torch.int32), col)
        z, W = torch.randn(B, d, device='cuda'), m.embedding_dict['W_dec'].detach()
        up = torch.full((B,), 1.0 / B, device='cuda')
        op = (lambda: mn.multinomial_softmax_kernel(z, W, P, up, want_grad=True, check_range=False)) if route == 'fused' else \
            (lambda: mn.multinomial_softmax_composed(z, W, P, up, want_grad=True))
        rec.step(rows, keep, eps, opt)                               # fills every gradient and Adam's state
        t = alternating({'step': lambda: rec.step(rows, keep, eps, opt), 'op': op, 'optimizer': opt.step}, reps, inner)
        r = {k: v['median_s'] for k, v in t.items()}
        r['encoder_and_rest_s'] = r['step'] - r['op'] - r['optimizer']
        r.update(share_op=r['op'] / r['step'], share_optimizer=r['optimizer'] / r['step'], share_encoder_and_rest=r['encoder_and_rest_s'] / r['step'],
                 step_min_s=t['step']['min_s'], step_max_s=t['step']['max_s'], step_peak_bytes=peak_above(lambda: rec.step(rows, keep, eps, opt)))
        out[route] = r
    out['step_speedup_median'] = out['composed']['step'] / out['fused']['step']
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=tuple(SHAPES) + ('all',), default='all')
    ap.add_argument('--legs', choices=('op', 'step', 'both'), default='both')
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=0)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'multvae_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('multvae_bench: needs the GPU; nothing here is measured on the CPU')
    lines = []
    for name in (tuple(SHAPES) if a.shape == 'all' else (a.shape,)):
        for leg, fn in (('op', run_op), ('step', run_step)):
            if a.legs in (leg, 'both'):
                lines.append(fn(name, a.dim, a.reps, a.inner))
                print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, auto_min_elems=mn.MULTINOMIAL_AUTO_MIN_ELEMS, legs=lines), fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

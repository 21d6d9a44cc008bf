#!/usr/bin/env python3
"""GSPAttack's L_per: the streaming kernel (ops.bce_allpairs_loss) against the composed torch route (panels of 128 rows), forward and forward +
backward, at cfg2's shape (SYN-v1 1 M x 100 K, d 64, nnz 32 095 419) and at ml-1M's shape (6 040 x 3 706, nnz 1 000 209).  The positives are drawn
uniformly (the loss's cost does not depend on where they lie).  Prints one JSON line per shape.

    python tools/gsp_bench.py [--shape cfg2|ml1m|both|none --dim 64 --reps 3 --composed-rows 20000] [--generator ml1m|cfg2|big|all]

--generator adds the profile generator's legs (pair-MLP logits + relaxed Gumbel top-k, forward + backward, csrc/arl_profilegen.hip): the fused and
the composed route in the same run at ml-1M's default budget (F 60, I 3 706, k 165, H 60) and at cfg2 with the bench's block of fake users (F 64,
I 100 000, k 32, H 316), and the fused route alone with hash noise at cfg2's default budget (F 10 000), with its peak memory.

The composed route at cfg2's size takes minutes (7 813 panels of 128 x 100 000 scores), so it is timed on the first --composed-rows rows and scaled
linearly in R (its cost per panel does not depend on R)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                  # noqa: E402
from arlib_amd import ops                     # noqa: E402

SHAPES = {'cfg2': (1_000_000, 100_000, 32_095_419), 'ml1m': (6040, 3706, 1_000_209)}
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


def positives(R, I, nnz, g):
    deg = torch.full((R,), nnz // R, dtype=torch.int64, device='cuda')
    deg[:nnz % R] += 1
    rowptr = torch.zeros(R + 1, dtype=torch.int32, device='cuda')
    rowptr[1:] = deg.cumsum(0).to(torch.int32)
    return rowptr, torch.randint(0, I, (nnz,), device='cuda', generator=g, dtype=torch.int32)


def run(name, d, reps, composed_rows):
    R, I, nnz = SHAPES[name]
    g = torch.Generator(device='cuda').manual_seed(0)
    Pu, Pi = torch.randn(R, d, device='cuda', generator=g) * 0.1, torch.randn(I, d, device='cuda', generator=g) * 0.1
    pos = positives(R, I, nnz, g)
    rw = ops.batch_mean_row_weights(R, I, device='cuda')
    pos_t = ops.transpose_positives(pos[0], pos[1], R, I)
    out = dict(shape=name, rows=R, items=I, dim=d, nnz=nnz)
    out['kernel_loss_s'] = timed(lambda: ops.bce_allpairs_loss(Pu, Pi, pos, rw, check_range=False), reps)
    out['kernel_loss_grad_s'] = timed(lambda: ops.bce_allpairs_loss(Pu, Pi, pos, rw, want_grad=True, pos_t=pos_t, check_range=False), reps)
    flop = 2.0 * R * I * d
    out['kernel_loss_tflops'] = flop / out['kernel_loss_s'] / 1e12                     # one score pass
    out['kernel_loss_grad_tflops'] = 4 * flop / out['kernel_loss_grad_s'] / 1e12       # two score passes, two weighted row sums
    out['kernel_loss_grad_share_of_fp32_matrix_peak'] = out['kernel_loss_grad_tflops'] / PEAK_TFLOPS
    Rc = min(R, composed_rows)
    sub = (pos[0][:Rc + 1].contiguous(), pos[1][:int(pos[0][Rc])].contiguous())
    Pus, rws = Pu[:Rc].contiguous(), rw[:Rc].contiguous()
    out['composed_rows_timed'] = Rc
    out['composed_loss_s_scaled'] = timed(lambda: ops.bce_allpairs_loss_composed(Pus, Pi, sub, rws, check_range=False), 1) * R / Rc
    out['composed_loss_grad_s_scaled'] = timed(lambda: ops.bce_allpairs_loss_composed(Pus, Pi, sub, rws, want_grad=True, check_range=False), 1) * R / Rc
    out['speedup_loss'] = out['composed_loss_s_scaled'] / out['kernel_loss_s']
    out['speedup_loss_grad'] = out['composed_loss_grad_s_scaled'] / out['kernel_loss_grad_s']
    print(json.dumps(out), flush=True)


GEN_SHAPES = {'ml1m': dict(F=60, I=3706, k=165, H=60), 'cfg2': dict(F=64, I=100_000, k=32, H=316), 'big': dict(F=10_000, I=100_000, k=32, H=316)}


def run_generator(name, d, reps):
    from torch.utils.checkpoint import checkpoint
    from arlib_amd.attack.Black.GSPAttack import MLP, gumbel_topk_relaxed
    F, I, k, H = (GEN_SHAPES[name][n] for n in 'FIkH')
    g = torch.Generator(device='cuda').manual_seed(0)
    Ef, Ei = torch.randn(F, d, device='cuda', generator=g) * 0.1, torch.randn(I, d, device='cuda', generator=g) * 0.1
    torch.manual_seed(0)
    mlp = MLP(2 * d, H).cuda()
    lin1, lin2 = mlp.net[0], mlp.net[2]
    up = torch.randn(F, I, device='cuda', generator=g)
    out = dict(leg='generator', shape=name, fake_users=F, items=I, k=k, hidden=H, dim=d)

    def fused(**src):
        mlp.zero_grad(set_to_none=True)
        A = Ef @ lin1.weight[:, :d].t() + lin1.bias
        B = Ei @ lin1.weight[:, d:].t()
        S, _ = ops.gumbel_topk(ops.pair_mlp_logits(A, B, lin2.weight[0], lin2.bias), k, **src)
        S.backward(up)

    def composed(noise):
        mlp.zero_grad(set_to_none=True)
        one = lambda u_row: mlp(torch.cat([u_row.expand(I, -1), Ei], 1))[:, 0]
        x = torch.stack([checkpoint(one, Ef[f], use_reentrant=False) for f in range(F)], 0)
        S, _ = gumbel_topk_relaxed(x, k, noise=noise)
        S.backward(up)
    if name == 'big':
        torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out['fused_hash_fwd_bwd_s'] = timed(lambda: fused(seed=1, call=0), 1)
        out['fused_hash_peak_bytes'] = torch.cuda.max_memory_allocated() - base
        out['composed_noise_and_softmax_bytes'] = 2 * k * F * I * 4
    else:
        noise = -torch.empty(k, F, I, device='cuda').exponential_(generator=g).log()
        out['fused_fwd_bwd_s'] = timed(lambda: fused(noise=noise), reps)
        out['fused_hash_fwd_bwd_s'] = timed(lambda: fused(seed=1, call=0), reps)
        out['composed_fwd_bwd_s'] = timed(lambda: composed(noise), reps)
        out['speedup_fwd_bwd'] = out['composed_fwd_bwd_s'] / out['fused_fwd_bwd_s']
        A = (Ef @ lin1.weight[:, :d].t() + lin1.bias).detach()
        B = (Ei @ lin1.weight[:, d:].t()).detach()
        w2, b2 = lin2.weight[0].detach(), lin2.bias.detach()
        x = ops.pair_mlp_fwd(A, B, w2, b2)
        out['pair_mlp_fwd_s'] = timed(lambda: ops.pair_mlp_fwd(A, B, w2, b2), reps)
        out['pair_mlp_bwd_s'] = timed(lambda: ops.pair_mlp_bwd(up, A, B, w2, b2), reps)
        _, picks, _, stats = ops.gumbel_topk_fwd(x, k, noise=noise)
        out['gumbel_fwd_s'] = timed(lambda: ops.gumbel_topk_fwd(x, k, noise=noise), reps)
        out['gumbel_bwd_s'] = timed(lambda: ops.gumbel_topk_bwd(up, x, k, picks, stats, noise=noise), reps)
        out['gumbel_hash_fwd_s'] = timed(lambda: ops.gumbel_topk_fwd(x, k, seed=1), reps)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('cfg2', 'ml1m', 'both', 'none'), default='both')
    ap.add_argument('--generator', choices=('none', 'ml1m', 'cfg2', 'big', 'all'), default='none')
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--composed-rows', type=int, default=20000)
    a = ap.parse_args()
    for name in (('ml1m', 'cfg2') if a.shape == 'both' else () if a.shape == 'none' else (a.shape,)):
        run(name, a.dim, a.reps, a.composed_rows)
    for name in (('ml1m', 'cfg2', 'big') if a.generator == 'all' else () if a.generator == 'none' else (a.generator,)):
        run_generator(name, a.dim, a.reps)


if __name__ == '__main__':
    main()

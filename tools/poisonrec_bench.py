#!/usr/bin/env python3
"""PoisonRec's policy head (csrc/arl_policyhead.hip) against the composed torch route, and the policy's share of one PPO rollout, at ml-1M's default
budget (F 60 fake users, I 3 706 items, d 64) and at cfg2's (F 10 000, I 100 000, d 64).  Prints one JSON line per leg and writes them all to
profiles/poisonrec_bench.json.

    python tools/poisonrec_bench.py [--shape ml1m|cfg2|both --reps 5 --rollout ml1m|cfg2|both|none --out profiles/poisonrec_bench.json]

Legs per shape:
  head     evaluation forward + backward (logp, ent, dq, dE), kernel and composed on the same inputs: wall time (host clock around a device
           synchronise, best of --reps after a warm-up) and peak device memory above the inputs; the kernel's rate against the exact-fp32 matrix
           peak (its four passes cost 12 B I d flop: four score products and two weighted row sums); both routes' errors against float64 (the whole
           problem at ml-1M's shape, the first 128 rows at cfg2's, where a float64 B x I matrix would take 8 GB)
  sample   the sampling pass at B = 1 (the rollout's step) and at B = F, with the caller's uniforms and with the counter hash
  rollout  one whole rollout + update of the attack on a SYN-v1 data set of the shape's size with a LightGCN victim: wall time of the rollout, of
           the retraining + scoring inside it (the environment's own clock, synchronised) and of the PPO update
A run without a GPU fails: nothing here is measured on the CPU."""
import argparse
import contextlib
import io
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                            # noqa: E402
import torch                                  # noqa: E402
from arlib_amd import ops                     # noqa: E402

SHAPES = {'ml1m': dict(F=60, I=3706, U=6040, deg=165.6), 'cfg2': dict(F=10_000, I=100_000, U=1_000_000, deg=32.0)}
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


def peak_above(fn):
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max().clamp_min(1e-30))


def float64_head(q, E, a, gl, ge):
    q, E = q.double().cpu().requires_grad_(), E.double().cpu().requires_grad_()
    p = torch.softmax(q @ E.t(), 1)
    sp = torch.log1p(torch.exp(p))
    logp, ent = (a.double().cpu() * p - sp).sum(1), (sp - p / (1 + torch.exp(-p))).sum(1)
    (gl.double().cpu() * logp + ge.double().cpu() * ent).sum().backward()
    return logp.detach(), ent.detach(), q.grad, E.grad


def problem(F, I, d, g):
    q, E = torch.randn(F, d, device='cuda', generator=g) * 0.3, torch.randn(I, d, device='cuda', generator=g)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (F, (I + 31) // 32), device='cuda', generator=g, dtype=torch.int64).to(torch.int32)
    if I % 32:
        words[:, -1] &= (1 << (I % 32)) - 1
    return q, E, words, torch.randn(F, device='cuda', generator=g), torch.randn(F, device='cuda', generator=g)


def run_head(name, d, reps):
    F, I = SHAPES[name]['F'], SHAPES[name]['I']
    g = torch.Generator(device='cuda').manual_seed(0)
    q, E, words, gl, ge = problem(F, I, d, g)
    out = dict(leg='head', shape=name, fake_users=F, items=I, dim=d)
    kern = lambda: ops.bernoulli_softmax_eval(q, E, words, gl, ge, want_grad=True)
    comp = lambda: ops.bernoulli_softmax_eval_composed(q, E, words, gl, ge, want_grad=True)
    out['kernel_fwd_bwd_s'], out['composed_fwd_bwd_s'] = timed(kern, reps), timed(comp, max(1, reps // 2))
    out['kernel_fwd_s'] = timed(lambda: ops.bernoulli_softmax_eval(q, E, words), reps)
    out['speedup_fwd_bwd'] = out['composed_fwd_bwd_s'] / out['kernel_fwd_bwd_s']
    out['kernel_peak_bytes'], out['composed_peak_bytes'] = peak_above(kern), peak_above(comp)
    out['one_fp32_F_x_I_matrix_bytes'] = 4 * F * I
    out['kernel_tflops'] = 12.0 * F * I * d / out['kernel_fwd_bwd_s'] / 1e12
    out['kernel_share_of_fp32_matrix_peak'] = out['kernel_tflops'] / PEAK_TFLOPS
    n = min(F, 128 if name == 'cfg2' else F)
    sub = [t[:n].contiguous() for t in (q, words, gl, ge)]
    want = float64_head(sub[0], E, ops.unpack_bits(sub[1], I), sub[2], sub[3])
    k = ops.bernoulli_softmax_eval(sub[0], E, sub[1], sub[2], sub[3], want_grad=True)
    c = ops.bernoulli_softmax_eval_composed(sub[0], E, sub[1], sub[2], sub[3], want_grad=True)
    out['error_rows'] = n
    for nm, a, b, w in zip(('logp', 'ent', 'dq', 'dE'), k, c, want):
        out['kernel_err_' + nm], out['composed_err_' + nm] = rel(a, w), rel(b, w)
    return out


def run_sample(name, d, reps):
    F, I = SHAPES[name]['F'], SHAPES[name]['I']
    g = torch.Generator(device='cuda').manual_seed(1)
    q, E, _, _, _ = problem(F, I, d, g)
    q1 = q[:1].contiguous()
    u1 = torch.rand(1, I, device='cuda', generator=g)
    out = dict(leg='sample', shape=name, fake_users=F, items=I, dim=d)
    out['kernel_B1_uniforms_s'] = timed(lambda: ops.bernoulli_softmax_sample(q1, E, u=u1), reps * 4)
    out['kernel_B1_hash_s'] = timed(lambda: ops.bernoulli_softmax_sample(q1, E, seed=1, call=0), reps * 4)
    out['composed_B1_uniforms_s'] = timed(lambda: ops.bernoulli_softmax_sample_composed(q1, E, u=u1), reps * 4)
    out['kernel_BF_hash_s'] = timed(lambda: ops.bernoulli_softmax_sample(q, E, seed=1, call=0), reps)
    out['kernel_BF_deterministic_s'] = timed(lambda: ops.bernoulli_softmax_sample(q, E, deterministic=True), reps)
    out['composed_BF_hash_s'] = timed(lambda: ops.bernoulli_softmax_sample_composed(q, E, seed=1, call=0), max(1, reps // 2))
    out['kernel_BF_hash_peak_bytes'] = peak_above(lambda: ops.bernoulli_softmax_sample(q, E, seed=1, call=0))
    return out


def run_rollout(name, d):
    from arlib_amd.util import synthetic
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.util.tool import seedSet
    from arlib_amd.recommender.LightGCN import LightGCN
    from arlib_amd.attack.Black.PoisonRec import PoisonRec
    S = SHAPES[name]
    U, I, F = S['U'], S['I'], S['F']
    p = np.asarray(synthetic.syn_v1_pairs_native(U, I, S['deg'], 2018))
    keep = np.ones(len(p), bool)
    keep[::97] = False                                                        # a thin test split; every user keeps most of its pairs for training
    ones = lambda a: np.ones(len(a), np.float32)
    tr, te = p[keep], p[~keep]
    data = DataLoader.from_arrays((tr[:, 0], tr[:, 1], ones(tr)), (te[:, 0], te[:, 1], ones(te)), (te[:, 0], te[:, 1], ones(te)), dataName='syn-' + name)
    seedSet(2018)
    rec = LightGCN(SimpleNamespace(dataset='syn-' + name, model_name='LightGCN', maxEpoch=1, batch_size=2048, emb_size=d, n_layers=3, reg=1e-4, lRate=0.005,
                                   seed=2018, topK='50'), data)
    with contextlib.redirect_stdout(io.StringIO()):
        rec.train(Epoch=1, evalNum=5)
    arg = SimpleNamespace(maliciousUserSize=F, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)
    atk = PoisonRec(arg, data, dim=d)
    out = dict(leg='rollout', shape=name, users=data.user_num, items=data.item_num, train_pairs=int(len(tr)), fake_users=F, dim=d,
               policy_route=atk.policy_route, feedback_per_fake_user=atk.maliciousFeedbackNum)
    with contextlib.redirect_stdout(io.StringIO()):
        atk.fakeUserInject(rec)
        atk._build(rec)
        ppo = atk.agent
        for n in range(2):                                                   # the first rollout + update warms every shape up; the second is reported
            atk.env.retrain_seconds = 0.0
            torch.cuda.synchronize(); t0 = time.perf_counter()
            ppo.collect_rollout()
            torch.cuda.synchronize(); t1 = time.perf_counter()
            log = ppo.train()
            torch.cuda.synchronize(); t2 = time.perf_counter()
    out['rollout_s'], out['retrain_and_scoring_s'], out['update_s'] = t1 - t0, atk.env.retrain_seconds, t2 - t1
    out['rollout_policy_and_environment_s'] = out['rollout_s'] - out['retrain_and_scoring_s']
    out['update_epochs'], out['update_stopped_by_kl'] = log['epochs'], log['stopped']
    total = out['rollout_s'] + out['update_s']
    out['share_retrain_and_scoring'] = out['retrain_and_scoring_s'] / total
    out['share_policy'] = 1.0 - out['share_retrain_and_scoring']
    out['share_update'] = out['update_s'] / total
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=('ml1m', 'cfg2', 'both'), default='both')
    ap.add_argument('--rollout', choices=('ml1m', 'cfg2', 'both', 'none'), default='ml1m')
    ap.add_argument('--dim', type=int, default=64)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles', 'poisonrec_bench.json'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('poisonrec_bench: needs the GPU; nothing here is measured on the CPU')
    lines = []
    for name in (('ml1m', 'cfg2') if a.shape == 'both' else (a.shape,)):
        for leg in (run_head, run_sample):
            lines.append(leg(name, a.dim, a.reps))
            print(json.dumps(lines[-1]), flush=True)
    for name in (('ml1m', 'cfg2') if a.rollout == 'both' else () if a.rollout == 'none' else (a.rollout,)):
        lines.append(run_rollout(name, a.dim))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, legs=lines), fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()

"""NCF / WRMF timings at cfg2 (1 M users + 100 K items, d = 64): the table-form tower kernel against the same three layers through
torch.nn.functional.linear + relu, and one NCF and one WRMF training step (train_batches, torch.optim.Adam).  Prints one JSON line.

    python tools/ncf_bench.py [--reps 20] [--legs tower,torch,ncf,ncf_tb,wrmf]

`--legs ncf` alone is the form to run under `rocprofv3 --kernel-trace --stats`: its trace holds the NCF training step's kernels only.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch                                                   # noqa: E402
import torch.nn.functional as F                                # noqa: E402


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
    ap.add_argument('--legs', default='tower,torch,ncf,ncf_tb,wrmf')
    a = ap.parse_args()
    legs = set(a.legs.split(','))
    from arlib_amd import ops
    from arlib_amd.recommender.NCF import NCF
    from arlib_amd.recommender.WRMF import WRMF
    U, I, d, B = a.users, a.items, 64, 2048
    args = SimpleNamespace(emb_size=d, topK='50', reg=1e-4, lRate=0.001, batch_size=B, maxEpoch=1)
    data = SimpleNamespace(user_num=U, item_num=I)
    torch.manual_seed(0)
    ncf = NCF(args, data)
    m = ncf.model.cuda()
    mf, mlp = m._pack()
    W = tuple(w.detach() for w in m._weights())
    N = U + I
    res = {'users': U, 'items': I, 'd': d}
    if 'tower' in legs:
        res['tower_table_ms'] = timed(lambda: ops.ncf_tower_fwd(mf, mlp, W), a.reps)
        res['tower_tflops'] = 2.0 * N * 17 * d * d / res['tower_table_ms'] / 1e9
        res['tower_fraction_of_157tf'] = res['tower_tflops'] / 157.0

    def torch_route():
        x = mlp
        for k in range(3):
            x = F.relu(F.linear(x, W[2 * k], W[2 * k + 1]))
        return torch.cat([mf, x], 1)
    if 'torch' in legs:
        with torch.no_grad():
            res['tower_torch_ms'] = timed(torch_route, a.reps)
    g = torch.Generator().manual_seed(1)
    batch = lambda: [(torch.randint(0, U, (B,), generator=g).numpy(), torch.randint(0, I, (B,), generator=g).numpy(),
                      torch.randint(0, I, (B,), generator=g).numpy())]
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    # one training step as _train_loop runs it (rows form on the batch's 3B rows), and as train_batches runs it (full-table forward)
    from arlib_amd.util.loss import bpr_l2_loss, wrmf_l2_loss
    bt = lambda: tuple(torch.randint(0, n, (B,), device='cuda', dtype=torch.int32) for n in (U, I, I))

    def rows_step(rec, opt, loss_fn):
        u, p, n = bt()
        out = rec.model.forward_rows(torch.cat([u, p + U, n + U]))
        loss = loss_fn(out[:B], out[B:2 * B], out[2 * B:], 1e-4)
        opt.zero_grad()
        loss.backward()
        opt.step()
    if 'ncf' in legs:
        res['ncf_step_rows_ms'] = timed(lambda: rows_step(ncf, opt, bpr_l2_loss), a.reps)
    if 'ncf_tb' in legs:
        res['ncf_step_train_batches_ms'] = timed(lambda: ncf.train_batches(batch(), opt), max(3, a.reps // 4))
    del opt, ncf, m, mf, mlp
    torch.cuda.empty_cache()
    wrmf = WRMF(args, data)
    wm = wrmf.model.cuda()
    wopt = torch.optim.Adam(wm.parameters(), lr=1e-3)
    if 'wrmf' in legs:
        res['wrmf_step_rows_ms'] = timed(lambda: rows_step(wrmf, wopt, wrmf_l2_loss), a.reps)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == '__main__':
    main()

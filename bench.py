#!/usr/bin/env python3
"""bench.py -- BPR-train interactions/sec of the LightGCN (d=64, L=3) + BPR + Adam step on the SYN-v1 synthetic
1M-user x 100K-item graph (BASELINE.json configs[1]), on N MI355X GPUs of one node.

  python bench.py --gpus 1 --steps K --warmup W [--dump-outputs DIR]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One "step" = one iteration of the reference's training inner loop (recommender/LightGCN.py:47-64) at the reference's
default batch size B = 2048: full-graph propagation, BPR + L2 loss on the batch, backward, dense Adam on both tables.
Batches are produced by the bit-exact host sampler before the timed region and are resident in HBM when it starts.
Prints ONE JSON line (rank 0).  The CPU baseline leg (rank 0, N=1 only) times the oracle's OpenMP restatement of the
same step on a bounded number of steps; the oracle is never on the measured GPU path.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md: HBM3E 8 TB/s (spec)
TRAFFIC_BLOCKED, TRAFFIC_CSR = 'r04_pmc_traffic_blocked.json', 'r01_pmc_traffic.json'      # PMC passes `roofline.traffic` quotes (tools/pmc_traffic.py)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--mean-deg', type=float, default=32.0)
    ap.add_argument('--emb', type=int, default=64)
    ap.add_argument('--layers', type=int, default=3)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--seed', type=int, default=2018)
    ap.add_argument('--chunk', type=int, default=512)
    ap.add_argument('--cpu-baseline', type=int, default=1, help='0 disables the CPU baseline leg')
    ap.add_argument('--cpu-seconds', type=float, default=12.0, help='target seconds of CPU work for the baseline sample')
    ap.add_argument('--cpu-torch', type=int, default=1, help='also time N steps of stock PyTorch-CPU running the reference-shaped math (COO sparse.mm + autograd + Adam)')
    ap.add_argument('--no-kernel-events', action='store_true', help='do not bracket SpMM launches with HIP events')
    ap.add_argument('--attack-steps', type=int, default=5, help='PGA gradient steps to time at N=1 (0 disables the attack leg)')
    ap.add_argument('--fake-users', type=int, default=64)
    ap.add_argument('--clear-steps', type=int, default=15, help='CLeaR surrogate steps to time at N=1 (median and spread are printed)')
    ap.add_argument('--schedule', default='auto', choices=['auto', 'csr', 'blocked'], help='full-graph hop schedule (engine.PropagationEngine)')
    ap.add_argument('--repeats', type=int, default=3, help='timed regions of K steps each: the first is the contract figure (`value`), all are listed with median and spread')
    ap.add_argument('--api-steps', type=int, default=600, help='steps of LightGCN(args, DataLoader).train() to time through the class API at N=1 (0 disables)')
    ap.add_argument('--model-steps', type=int, default=20, help='steps of the SimGCL (L=2) and NGCF (d=128, L=3) training steps to time at N=1 on the same graph (0 disables)')
    ap.add_argument('--share-steps', type=int, default=30, help='steps of ONE rank\'s share of the N=8 step to time alone on this GPU (projected_ceiling_8gpu; 0 disables)')
    ap.add_argument('--l2-ceiling', type=int, default=1, help='measure the hop with every gather an L2 hit (roofline.attainable); 0 disables')
    ap.add_argument('--dense-step', action='store_true', help='time the reference-shaped step (all 2L hops on the full graph) as the main number')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='after the timed steps write what the last one computed as DIR/<name>.npy (loss vector, seeded sample of the table rows; '
                         'at most 64 MB): two builds run with the same arguments can be compared output for output')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')
    return args


DUMP_BYTES = 64 * 10**6        # --dump-outputs: bytes of all arrays together


def dump_rows(U, I, d, seed):
    """Rows of the [U+I, d] table that --dump-outputs writes: all of them if the table fits DUMP_BYTES, otherwise a sample drawn from `seed`
    alone (every item row if the items fit in half the budget, user rows fill the rest), sorted.  The same arguments give the same rows."""
    budget = (DUMP_BYTES - 4096) // (4 * d)                  # rows; 4 KB for the loss vector and the .npy headers
    n_i = min(I, max(budget // 2, budget - U))
    n_u = min(U, budget - n_i)
    rng = np.random.default_rng(seed)
    pick = lambda n_all, n: np.arange(n_all, dtype=np.int64) if n == n_all else np.sort(rng.choice(n_all, n, replace=False)).astype(np.int64)
    return pick(U, n_u), pick(I, n_i)


def capture_outputs(torch, eng, lo, U, I, d, seed, sharded):
    """What a caller of the timed step holds after its last call: the loss vector it returned ([bpr, reg term, ||U_b||, ||P_b||]) and the updated
    embedding table, as host arrays (table rows: dump_rows).  Under sharding every rank contributes its own user rows; the item rows are replicated."""
    rows_u, rows_i = dump_rows(U, I, d, seed)
    take = lambda rows: eng.E0.index_select(0, torch.from_numpy(rows).to(eng.E0.device)).cpu().numpy()
    loss = lo.detach().cpu().numpy().astype(np.float32)
    if not sharded:
        return {'loss': loss, 'user_emb': take(rows_u), 'item_emb': take(U + rows_i)}
    import torch.distributed as dist
    mine = rows_u[(rows_u >= eng.u0) & (rows_u < eng.u1)]
    parts = [None] * dist.get_world_size()
    dist.all_gather_object(parts, (mine, take(mine - eng.u0)))
    rows = np.concatenate([p[0] for p in parts])
    user = np.concatenate([p[1] for p in parts])[np.argsort(rows, kind='stable')]
    return {'loss': loss, 'user_emb': user, 'item_emb': take(eng.Ul + rows_i)}


def write_outputs(out_dir, arrays):
    os.makedirs(out_dir, exist_ok=True)
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_BYTES and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)
    return {name: list(a.shape) for name, a in arrays.items()}


class SpmmEvents:
    """HIP events around every SpMM-family launch in the timed region (same stream as the kernels)."""

    def __init__(self, torch):
        self.torch = torch
        self.recs = []
        self.on = False
        self.calls_seen = 0          # launches counted while off (the warm-up steps): sizes the pool
        self.pool = []

    def prepare(self, n_events):
        """Create the events BEFORE the timed region (an event's first record() creates the HIP object: ~5 us each, ~16 per step inside the region
        otherwise); recording an existing event again costs next to nothing."""
        self.pool = [self.torch.cuda.Event(enable_timing=True) for _ in range(n_events)]
        for e in self.pool:
            e.record()
        self.torch.cuda.synchronize()

    def _event(self):
        return self.pool.pop() if self.pool else self.torch.cuda.Event(enable_timing=True)

    def begin(self, tag):
        if not self.on:
            self.calls_seen += 1
            return None
        s = self._event()
        s.record()
        return (tag, s)

    def end(self, tok):
        if tok is None:
            return
        e = self._event()
        e.record()
        self.recs.append((tok[0], tok[1], e))

    def summary(self):
        out = {}
        for tag, s, e in self.recs:
            out.setdefault(tag, []).append(s.elapsed_time(e))
        return {k: (float(np.mean(v)), len(v)) for k, v in out.items()}


def l2_ceiling(torch, ops, rowptr, col, U, d, dev, chunk, reps=10):
    """The hop's attainable time on this schedule: the SAME plan builder, records, waves and instruction stream with every column folded into a
    2 MB window of the operand (col & 8191), so that every 256-B row gather is an L2 hit.  What remains is the L2 -> CU gather rate the
    microarchitecture guide quotes for L2-resident rows (66-73 GB/s per CU); HBM-side bytes no longer matter.  Returns ms per full-graph hop."""
    import ctypes as C
    from arlib_amd import _lib
    c = col.copy()
    eu = int(rowptr[U])
    c[:eu] = U + ((c[:eu] - U) & 8191)
    c[eu:] = c[eu:] & 8191
    N = len(rowptr) - 1
    A = ops.CSRGraph(rowptr, c, np.ones(len(c), np.float32), dev, chunk=chunk, validate=False).enable_blocked(split=U)
    X = torch.randn(N, d, device=dev); Y = torch.empty(N, d, device=dev)
    st = ops._stream()
    structs = [A.blocked.struct(k, d) for k in range(len(A.blocked.sets))]

    def hop():
        for s in structs:
            _lib.check(_lib.lib().arl_spmm_blocked_f32(C.byref(s), X.data_ptr(), d, 1.0, 0.0, None, None, Y.data_ptr(), st), 'arl_spmm_blocked_f32')
    for _ in range(3):
        hop()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        hop()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def cpu_baseline(data, rowptr, col, val_np, E0, batches, args, target_s, gpu_replay=None):
    """Oracle ('port') timed on the host cores: same graph, same tables, same batches, OpenMP over rows."""
    from oracle import oracle as O
    O.build()
    U, I = data.user_num, data.item_num
    st = O.TrainState(E0[:U], E0[U:], (rowptr, col, val_np), args.layers, 1e-4, 0.005)
    st.f32acc = True
    done, t_used = 0, 0.0
    max_steps = min(len(batches), 8)
    while done < max_steps and (t_used < target_s or done < 1):
        b = batches[done]
        t0 = time.perf_counter()
        st.step(b[0], b[1], b[2])
        t_used += time.perf_counter() - t0
        done += 1
    out = {'value': args.batch * done / t_used, 'unit': 'interactions/s', 'cores': O.num_threads(), 'kind': 'port',
           'sample': '%d full training steps of the same workload (same graph, tables and batches), %.1f s of CPU work, '
                     'oracle/arl_oracle.c with OpenMP over rows' % (done, t_used),
           'ms_per_step': 1e3 * t_used / done}
    if gpu_replay is not None:
        # the same `done` steps from the same start on the GPU engine: the full-size parity figure (the suite's size-independent
        # properties aside, this is the one place where product and oracle meet at cfg2)
        table = gpu_replay(done)
        ref = st.E0
        out['parity_vs_gpu'] = {'steps': done, 'table_rel_err': float(np.linalg.norm(table - ref) / np.linalg.norm(ref)),
                                'max_abs_err': float(np.abs(table - ref).max())}
    return out


def cpu_torch_baseline(torch, rowptr, col, val_np, E0, batches, U, args, n_steps):
    """Stock PyTorch on the host cores executing the step the way the reference expresses it (recommender/LightGCN.py:230-252,
    util/loss.py:5-29): COO sparse tensor, L x torch.sparse.mm, stack + mean, BPR + L2, autograd backward, torch.optim.Adam.
    Reported beside the oracle port as SURVEY 8d asks; never the graded baseline."""
    N = len(rowptr) - 1
    rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    A = torch.sparse_coo_tensor(torch.from_numpy(np.stack([rows, col.astype(np.int64)])), torch.from_numpy(val_np), (N, N))
    ue, ie = torch.nn.Parameter(E0[:U].clone()), torch.nn.Parameter(E0[U:].clone())
    opt = torch.optim.Adam([ue, ie], lr=0.005)
    times = []
    for k in range(n_steps):
        u, p, n = (torch.from_numpy(b.astype(np.int64)) for b in batches[k])
        t0 = time.perf_counter()
        ego = torch.cat([ue, ie], 0)
        layers = [ego]
        for _ in range(args.layers):
            ego = torch.sparse.mm(A, ego)
            layers.append(ego)
        out = torch.stack(layers, 1).mean(1)
        eu, ep, en = out[u], out[U + p], out[U + n]
        loss = -torch.log(1e-7 + torch.sigmoid((eu * ep).sum(1) - (eu * en).sum(1))).mean() + 1e-4 * (torch.norm(eu, p=2) + torch.norm(ep, p=2))
        opt.zero_grad()
        loss.backward()
        opt.step()
        times.append(time.perf_counter() - t0)
    t = float(np.mean(times[1:])) if len(times) > 1 else times[0]
    return {'value': args.batch / t, 'unit': 'interactions/s', 'cores': torch.get_num_threads(), 'kind': 'stock PyTorch CPU, reference-shaped step',
            'ms_per_step': 1e3 * t, 'steps_timed': max(1, len(times) - 1), 'loss': float(loss.detach())}


def attack_leg(torch, ops, data, E0_dev, args):
    """attack-grad steps/sec (BASELINE metric, configs[2]): one step = one PGA iteration on the fake-interaction block
    (attack/White/PGA.py:92-142): device re-normalisation of the poisoned graph, L-hop forward, CW gradient (one SpMM with the
    bilinear operator), L-1 hop backward, 2L row-restricted SDDMMs, tanh/clamp update.  F fake users, T=5 unpopular targets."""
    import scipy.sparse as sp
    from arlib_amd.attack.White.PGA import FactoredFakeGraph, _hop, cw_operator, pga_step_block
    from arlib_amd.attack._common import cw_pairs
    U, I, nnz = data.training_size()
    F, L, d = args.fake_users, args.layers, args.emb
    t0 = time.perf_counter()
    real = sp.csr_matrix((np.ones(nnz, np.float32), (data.pairs0[:, 0], data.pairs0[:, 1])), shape=(U, I))
    deg_i = np.bincount(data.pairs0[:, 1], minlength=I)
    targets = [int(t) for t in np.argsort(deg_i, kind='stable')[:5]]
    popular = np.argsort(-deg_i, kind='stable')[:int(0.05 * I)]
    fg = FactoredFakeGraph(real, U, F, I, device=E0_dev.device, emb_size=None if args.schedule == 'csr' else d)
    del real
    S = torch.zeros(F, I, device=E0_dev.device)
    S[:, targets] = 1.0
    S[:, torch.from_numpy(popular).to(S.device)] = 0.5
    g = torch.Generator().manual_seed(args.seed)
    fake_tab = torch.nn.init.xavier_uniform_(torch.empty(F, d), generator=g).to(E0_dev.device)
    E0 = torch.cat([E0_dev[:U], fake_tab, E0_dev[U:]], 0).contiguous()
    setup_s = time.perf_counter() - t0
    graph = fg.set_block(S)
    out = E0.clone(); E = E0
    for k in range(L):
        E = _hop(graph, E); out += E
    out /= (L + 1)
    Pu_all, Pi_all = out[:U + F].contiguous(), out[U + F:].contiguous()
    ops.score_mask_topk(Pu_all[:256].contiguous(), Pi_all, 50)      # first call of the process: code-object load of the kernel and of torch's sort (not timed)
    topk_all = []
    ops.TOPK_STATS['record_exit'], ops.TOPK_STATS['exit'] = True, []      # early-exit counters of every pass (16-byte device copies; read after the timing)
    for _ in range(3):                               # three passes (the GPU has idled through the host-side set-up above: the first one also pays the clock ramp)
        torch.cuda.synchronize(); t1 = time.perf_counter()
        top_idx, _ = ops.score_mask_topk(Pu_all, Pi_all, 50)
        torch.cuda.synchronize(); topk_all.append(time.perf_counter() - t1)
    topk_s = sorted(topk_all)[1]                     # the median is the figure
    skipped_trained = ops.topk_exit_fractions()
    # the same pass on RANDOM tables of the same shape (no norm structure: the exit bound never holds, expected share skipped = 0)
    gr = torch.Generator(device=E0_dev.device).manual_seed(args.seed)
    Ru = torch.randn(Pu_all.shape, generator=gr, device=E0_dev.device); Ri = torch.randn(Pi_all.shape, generator=gr, device=E0_dev.device)
    ops.reset_exit_probe()                           # (new tables of the same shape: what the passes above learnt about the early exit does not carry over)
    ops.score_mask_topk(Ru, Ri, 50); torch.cuda.synchronize(); t1 = time.perf_counter()
    ops.score_mask_topk(Ru, Ri, 50); torch.cuda.synchronize(); topk_random_s = time.perf_counter() - t1
    skipped_random = ops.topk_exit_fractions()
    # ... and with the item rows' NORMS spread like a popularity-skewed model's (log-normal, sigma 1; same random directions): what the exit buys when the
    # tables have the structure it needs -- the device picks the exit build of the kernel from the norm profile, the plain one otherwise
    Ri *= torch.exp(torch.randn(Ri.shape[0], 1, generator=gr, device=E0_dev.device))
    ops.reset_exit_probe()
    ops.score_mask_topk(Ru, Ri, 50); torch.cuda.synchronize(); t1 = time.perf_counter()
    ops.score_mask_topk(Ru, Ri, 50); torch.cuda.synchronize(); topk_skewed_s = time.perf_counter() - t1
    skipped_skewed = ops.topk_exit_fractions()
    del Ru, Ri
    ops.TOPK_STATS['record_exit'] = False
    ops.reset_exit_probe()
    del Pu_all, Pi_all
    M = cw_operator(U + F + I, U + F, *cw_pairs(top_idx, U, targets, pop=True), device=E0.device)

    def step():
        gr = fg.set_block(S)
        block, loss = pga_step_block(gr, fg.fake_rows, U + F, I, E0, L, M)
        ops.pga_update_(S, block, fg.dinv[U:U + F].contiguous(), fg.dinv[U + F:].contiguous())
        return loss
    step(); torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(args.attack_steps):
        loss = step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t2) / args.attack_steps
    cpu = None
    if args.cpu_baseline:
        # the same PGA step through the oracle on the host cores: per-step graph rebuild + renormalisation (what PGA.py:93-97 does
        # with scipy), L-hop forward, CW gradient, L-1 hop backward, SDDMM block, tanh/clamp update -- one step, it takes seconds
        from oracle import oracle as O
        O.build()
        rowptr, col = data.adjacency_pattern()
        users_h, pos_h, neg_h = (t.cpu().numpy() for t in cw_pairs(top_idx, U, targets, pop=True))
        S_h, E0_h = S.cpu().numpy(), E0.cpu().numpy()
        cpu_times = []
        for _ in range(2):                           # first step warms the OpenMP team / page cache; the second is the figure
            tc = time.perf_counter()
            _, S_next, cw_h = O.pga_step(rowptr[:U + 1].astype(np.int64), (col[:nnz] - U).astype(np.int64), U, F, I, S_h, E0_h, L, users_h, pos_h, neg_h)
            cpu_times.append(time.perf_counter() - tc)
        cpu_s = cpu_times[-1]
        cpu = {'value': 1.0 / cpu_s, 'unit': 'steps/s', 'cores': O.num_threads(), 'kind': 'port', 'seconds_per_step': cpu_s, 'first_unwarmed_step_s': cpu_times[0],
               'sample': '1 PGA step of the same workload after 1 warm-up step (oracle: numpy graph rebuild + OpenMP SpMM + scipy CW product)', 'cw_loss': float(cw_h)}
    Ep, Np = 2 * nnz + 2 * F * I, U + F + I
    step_bytes = L * (8 * Ep + 4 * Np + 16 * Np * d) + (L - 1) * (8 * Ep + 4 * Np + 8 * Np * d) + L * (2 * F * I * 4 + 2 * I * d * 4 + 2 * F * d * 4) + 3 * F * I * 4
    return {'metric': 'attack-grad steps/sec (PGA gradient w.r.t. fake interactions, LightGCN d=%d L=%d surrogate)' % (d, L),
            'value': 1.0 / dt, 'unit': 'steps/s', 'ms_per_step': 1e3 * dt, 'fake_users': F, 'targets': 5, 'cw_loss': float(loss),
            'algorithmic_bytes_per_step': step_bytes, 'hbm_frac': step_bytes / dt / 1e9 / HBM_PEAK_GBS,
            'cpu_baseline': cpu,
            'score_topk_pass': {'seconds': topk_s, 'seconds_all': topk_all, 'tflops': 2.0 * (U + F) * I * d / topk_s / 1e12,
                                'roofline': {'bound': 'mfma', 'achieved': 2.0 * (U + F) * I * d / topk_s / 1e12, 'peak': 2500.0, 'unit': 'TFLOP/s',
                                             'frac': 2.0 * (U + F) * I * d / topk_s / 1e12 / 2500.0,
                                             'note': 'fp16 matrix flops executed by the stream: ONE fp16 product per (user, item, k) -- the high pieces; the two other products of '
                                                     'the split form run only for queued candidates (a 16 x 16 tile per merge) and are not counted; dense fp16/bf16 MFMA peak. '
                                                     'The pass is bound by its ring / candidate handling, not by the matrix pipe (DESIGN 3b)'},
                                'stages_skipped_frac': {'trained_propagated_tables': skipped_trained, 'random_tables': skipped_random, 'lognormal_item_norms': skipped_skewed,
                                                        'what': 'share of (workgroup, 64-item stage) pairs of the norm-ordered item stream the exact early exit never scored'},
                                'random_tables_seconds': topk_random_s, 'lognormal_item_norms_seconds': topk_skewed_s,
                                'note': '`tflops` = fp32-equivalent (2 U I d); once per inner epoch, not per step'},
            'setup_seconds': setup_s}


def clear_leg(torch, ops, data, A, E0_dev, args):
    """attack-grad steps/sec, CLeaR flavour (attack/White/CLeaR.py:73-129): one step = surrogate forward with grad, streaming
    U x I score + interacted-mask + top-k, CW over (real user x target) pairs + SFA L1 term on the gathered [3UT, d] matrix,
    backward through the propagation, Adam over both tables.  Surrogate = the clean cfg2 graph (the F appended rows of a
    poisoned graph change the cost by F/U)."""
    from types import SimpleNamespace
    from arlib_amd.recommender._base import GraphEncoder, SparseNormAdj
    from arlib_amd.attack.White.CLeaR import CLeaR
    U, I, nnz = data.training_size()
    L, d = args.layers, args.emb
    dev = E0_dev.device
    enc = GraphEncoder.__new__(GraphEncoder)
    torch.nn.Module.__init__(enc)
    enc.data = SimpleNamespace(user_num=U, item_num=I)
    enc.latent_size = enc.emb_size = d
    enc.n_prop_layers = L
    enc._eng = None
    packed = E0_dev.clone()
    enc.embedding_dict = torch.nn.ParameterDict({'user_emb': torch.nn.Parameter(packed[:U]), 'item_emb': torch.nn.Parameter(packed[U:])})
    adj = SparseNormAdj.__new__(SparseNormAdj)
    adj.shape, adj.indptr, adj.indices, adj.values, adj._graph = (U + I, U + I), None, None, A.val, A
    enc.sparse_norm_adj = adj
    rowptr, col = data.adjacency_pattern()
    mask = (torch.from_numpy(rowptr[:U + 1].astype(np.int32)).to(dev), torch.from_numpy((col[:nnz] - U).astype(np.int32)).to(dev))
    deg_i = np.bincount(data.pairs0[:, 1], minlength=I)
    atk = CLeaR.__new__(CLeaR)
    atk.userNum, atk.itemNum, atk.targetItem = U, I, [int(t) for t in np.argsort(deg_i, kind='stable')[:5]]
    from arlib_amd.util.optim import Adam                     # what CLeaR.posionDataAttack builds for its surrogate (torch.optim.Adam, stepped by arl_adam_dense_f32)
    opt = Adam(enc.parameters(), lr=0.005)
    r0 = torch.randn(d, generator=torch.Generator().manual_seed(args.seed)).to(dev)
    warm = [None]

    def step(ev=None):
        if ev is not None:
            ev[0].record()
        lossall, _, _, cw, sfa = atk.surrogate_loss(enc, mask, 50, r0=r0, warm=warm[0])       # steps after the first reuse the previous lists
        warm[0] = atk.last_top_idx
        if ev is not None:
            ev[1].record()
        opt.zero_grad()
        lossall.backward()
        opt.step()
        if ev is not None:
            ev[2].record()
        if os.environ.get('ARL_CLEAR_TRACE') == '1':                # diagnostics (synchronising): loss terms and table magnitudes per step
            trace.append((float(cw.detach()), float(sfa.detach()), float(enc.embedding_dict['user_emb'].detach().abs().max()), float(enc.embedding_dict['item_emb'].detach().abs().max())))
        return cw.detach(), sfa.detach()
    trace = []
    step(); step(); torch.cuda.synchronize()                 # a cold-started step and the first warm-started one (its own kernel instantiation: code-object load) are not timed
    n = max(1, args.clear_steps)
    # The timed loop never waits for the device (as the attack's own loop, CLeaR.py:73-129 / attack/White/CLeaR.py): step boundaries are HIP events on
    # the launch stream, the wall clock brackets all n steps between two synchronisations.  (Waiting for every step made the figure depend on how fast the
    # host thread wakes up after a 45 ms kernel: 58 ms per step on some boxes, 80-100 ms in 10 ms quanta on others, with the same device-side spans.)
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(n)]
    ops.TOPK_STATS['record_events'], ops.TOPK_STATS['events'], ops.TOPK_STATS['flags'] = True, [], []      # device-side span of every scoring pass of the timed steps
    ops.TOPK_STATS['record_exit'], ops.TOPK_STATS['exit'] = True, []
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for k in range(n):
        cw, sfa = step(evs[k])
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    ops.TOPK_STATS['record_events'] = ops.TOPK_STATS['record_exit'] = False
    skipped = ops.topk_exit_fractions()
    topk_dev = [a.elapsed_time(b) for a, b in ops.TOPK_STATS.pop('events', [])]
    cold_repeats = int(sum(int(f) != 0 for f in ops.TOPK_STATS.pop('flags', [])))
    per = [evs[k][0].elapsed_time(evs[k + 1][0]) * 1e-3 for k in range(n - 1)] + [evs[n - 1][0].elapsed_time(evs[n - 1][2]) * 1e-3]      # step start to next step start
    fwd = [e[0].elapsed_time(e[1]) for e in evs]
    return {'metric': 'attack-grad steps/sec (CLeaR surrogate step: CW + SFA, LightGCN d=%d L=%d)' % (d, L), 'value': 1.0 / dt, 'unit': 'steps/s',
            'ms_per_step': 1e3 * dt, 'steps_timed': n, 'ms_per_step_median': 1e3 * float(np.median(per)), 'ms_per_step_min': 1e3 * min(per), 'ms_per_step_max': 1e3 * max(per),
            'ms_per_step_all': [round(1e3 * x, 2) for x in per], 'topk_device_ms_all': [round(x, 2) for x in topk_dev], 'topk_device_ms_median': float(np.median(topk_dev)) if topk_dev else None,
            **({'trace_cw_sfa_umax_imax': trace} if trace else {}), 'topk_cold_repeats': cold_repeats, 'topk_stages_skipped_frac_all': [round(x, 4) for x in skipped],
            'ms_forward_topk_loss': float(np.mean(fwd)), 'targets': 5, 'pairs': U * 5,
            'cw_loss': float(cw), 'sfa_loss': float(sfa), 'score_flops_per_step': 2.0 * U * I * d,
            'timing': '`ms_per_step` = wall clock over the %d steps between two device synchronisations / %d; per-step figures = HIP events at the step boundaries on the launch stream' % (n, n),
            'note': 'dominated by the U x I scoring pass (compute-bound line item, SURVEY 8d): `topk_device_ms_all` is its device-side span per step; peak memory %.1f GB' % (torch.cuda.max_memory_allocated() / 1e9)}


def ncl_structure_leg(torch, E0_dev, args, reps=10):
    """NCL's structure-contrastive term at cfg2 sizes (recommender/NCL.py:96-115): the batch's 2 048 rows against ALL user rows and ALL item
    rows, forward + backward (row normalisation, log-sum-exp over the table, gradients to both sides), no B x N logit matrix."""
    from arlib_amd.recommender.NCL import all_rows_nce
    U, B, d = args.users, args.batch, args.emb
    g = torch.Generator().manual_seed(args.seed)
    out = {}
    for name, tab in (('users', E0_dev[:U]), ('items', E0_dev[U:])):
        N = tab.shape[0]
        V0 = tab.clone().requires_grad_(True)
        C0 = (tab + 0.05 * torch.randn(tab.shape, generator=g).to(tab.device)).requires_grad_(True)
        idx = torch.randint(0, N, (B,), generator=g).to(tab.device)

        def run():
            all_rows_nce(C0[idx], V0, idx, 0.05).backward()
            V0.grad = None; C0.grad = None
        for _ in range(2):
            run()
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t0) / reps
        out[name] = {'rows': N, 'ms': ms, 'tflops_fp32': 4 * 2.0 * B * N * d / (ms * 1e-3) / 1e12}
    out['what'] = 'all-rows InfoNCE of a %d-row batch, d=%d, temperature 0.05: forward + backward, 4 exact-fp32 MFMA passes of 2*B*N*d flop each' % (B, d)
    return out


def model_legs(torch, ops, engine, data, A, dev_batches, args, steps=20):
    """Driver-visible steps of BASELINE configs 4 and 5 on ONE GPU, same cfg2 graph and batches as the headline:
      simgcl_step -- SimGCL (recommender/SimGCL.py:51-70,198-219): three forwards (clean + two perturbed views, noise drawn inside the perturbation
                     kernel), BPR + L2 + InfoNCE at the batch's unique users / positive items, one backward, dense Adam; L = 2 (the reference hard-codes it, Q14);
      ngcf_step   -- NGCF d = 128, L = 3 (recommender/NGCF.py:47-64,197-212): per layer one hop + the fp32-MFMA dense part, BPR + L2, backward, Adam on
                     both tables and the 2L weight matrices.
    Algorithmic bytes per step (E = 2 nnz, N = U + I): SimGCL `3 L (16E + 8N + 24Nd) + 28Nd + 24Bd + 16 n^2` (n = batch size as the bound on the unique
    rows); NGCF `L (2 (8E + 4N + 8Nd) + 52Nd) + 28Nd + 24Bd` (per layer: the hop forward and backward, the dense part's 12Nd forward + 28Nd dgrad + 12Nd wgrad)."""
    U, I, nnz = data.training_size()
    N, E, B = U + I, 2 * nnz, args.batch
    dev = dev_batches.device
    out = {}
    g = torch.Generator().manual_seed(args.seed)

    def run(step_fn):
        for k in range(3):
            step_fn(k)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for k in range(3, 3 + steps):
            last = step_fn(k % dev_batches.shape[0])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps, last

    # ---- SimGCL, d = args.emb, L = 2
    d, L = args.emb, 2
    E0 = torch.cat([torch.nn.init.xavier_uniform_(torch.empty(U, d), generator=g), torch.nn.init.xavier_uniform_(torch.empty(I, d), generator=g)], 0).to(dev)
    eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, dev, skip_layer0=True, table=E0)
    dt, last = run(lambda k: eng.step_simgcl(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2]))
    by = 3 * L * (16 * E + 8 * N + 24 * N * d) + 28 * N * d + 24 * B * d + 16 * B * B
    out['simgcl_step'] = {'metric': 'BPR-train interactions/sec (SimGCL d=%d L=%d: 3 forwards + InfoNCE + Adam, B=%d)' % (d, L, B), 'value': B / dt, 'unit': 'interactions/s',
                          'ms_per_step': 1e3 * dt, 'steps_timed': steps, 'algorithmic_bytes_per_step': by, 'hbm_frac': by / dt / 1e9 / HBM_PEAK_GBS,
                          'rec_loss': float(last[0][0] + last[0][1]), 'cl_loss': float(last[1]),
                          'note': 'cfg2 graph; noise drawn in the perturbation kernel (the reference draws rand_like per hop and view); the shared first hop, row-subset last '
                                  'hops and the single backward pass make it 2 full hops + 1 masked + 3 row-subset hops instead of 12 full hops'}
    del eng, E0
    torch.cuda.empty_cache()
    # ---- NGCF, d = 128, L = 3
    d, L = 128, 3
    E0 = torch.cat([torch.nn.init.xavier_uniform_(torch.empty(U, d), generator=g), torch.nn.init.xavier_uniform_(torch.empty(I, d), generator=g)], 0).to(dev)
    eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, dev, table=E0)
    eng.init_ngcf([(torch.nn.init.xavier_uniform_(torch.empty(d, d), generator=g).to(dev), torch.nn.init.xavier_uniform_(torch.empty(d, d), generator=g).to(dev)) for _ in range(L)])
    rows = torch.cat([dev_batches[:, 0], dev_batches[:, 1] + U, dev_batches[:, 2] + U], 1).contiguous()
    dt, last = run(lambda k: eng.step_ngcf(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2], rows=rows[k]))
    by = L * (2 * (8 * E + 4 * N + 8 * N * d) + 52 * N * d) + 28 * N * d + 24 * B * d
    out['ngcf_step'] = {'metric': 'BPR-train interactions/sec (NGCF d=%d L=%d + BPR/L2 + Adam, B=%d)' % (d, L, B), 'value': B / dt, 'unit': 'interactions/s',
                        'ms_per_step': 1e3 * dt, 'steps_timed': steps, 'algorithmic_bytes_per_step': by, 'hbm_frac': by / dt / 1e9 / HBM_PEAK_GBS,
                        'loss': float(last[0] + last[1]), 'peak_memory_GB': torch.cuda.max_memory_allocated() / 1e9,
                        'note': 'cfg2 graph at the width of BASELINE config 5 (d = 128); fused route (engine.step_ngcf): no autograd, no torch optimizer'}
    del eng, E0, rows
    torch.cuda.empty_cache()
    return out


class _NullWork:
    def wait(self):
        return True


class _NullComm:
    """Stand-in collective for ONE rank's share timed alone on this GPU: the buffers are left as they are (the values of the item rows are then this
    rank's partials -- the kernels' cost does not depend on them), nothing is exchanged, nothing waits."""
    measure = False
    item_exchange = 'none'

    def all_reduce_async(self, t):
        return _NullWork()

    def all_reduce(self, t):
        return t


def share_leg(torch, data, E0, dev_batches, args, ms_1gpu, world=8, steps=30):
    """What bounds the 8-GPU speed-up before a byte crosses xGMI: rank 0's share of the cfg2 step at N = 8 (125 K local users x 100 K items: its two
    rectangular blocks, its batch samples, the replicated item table and Adam state) run through the SAME code path `bench.py --gpus 8` runs
    (dist_engine.ShardedPropagationEngine.step_sparse) with a no-op collective, timed alone on this GPU.  projected_ceiling_8gpu = t_1gpu / t_share: the
    strong-scaling speed-up with zero exposed communication and perfectly balanced ranks (SYN-v1 users are i.i.d., the blocks have equal size)."""
    from arlib_amd import dist_engine
    U, I, nnz = data.training_size()
    dev = dev_batches.device
    t0 = time.perf_counter()
    eng = dist_engine.ShardedPropagationEngine.from_pairs(data.pairs0, U, I, args.emb, args.layers, 1e-4, 0.005, dev, 0, world, table=E0, chunk=args.chunk,
                                                           schedule=args.schedule, comm=_NullComm())
    build_s = time.perf_counter() - t0
    nb = dev_batches.shape[0]
    for k in range(5):
        eng.step_sparse(dev_batches[k % nb, 0], dev_batches[k % nb, 1], dev_batches[k % nb, 2])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    th = time.perf_counter(); e0.record()
    for k in range(steps):
        eng.step_sparse(dev_batches[k % nb, 0], dev_batches[k % nb, 1], dev_batches[k % nb, 2])
    e1.record(); t_enq = time.perf_counter() - th
    torch.cuda.synchronize()
    span_ms = e0.elapsed_time(e1) / steps
    # GPU-busy time and launch count per step from the profiler's device records (the span above also holds launch gaps)
    busy_ms = launches = None
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for k in range(3):
                eng.step_sparse(dev_batches[k % nb, 0], dev_batches[k % nb, 1], dev_batches[k % nb, 2])
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        busy_ms, launches = sum(e.device_time for e in ev) / 3e3, len(ev) / 3.0
    except Exception as e:                                   # the figure of merit below falls back to the event span
        busy_ms = None
    t_share = busy_ms if busy_ms else span_ms
    del eng
    torch.cuda.empty_cache()
    return {'what': 'rank 0 of %d: %d local users x %d items, same step as --gpus %d (step_sparse), no-op collective, alone on this GPU' % (world, U // world, I, world),
            'gpu_busy_ms_per_step': busy_ms, 'launches_per_step': launches, 'event_span_ms_per_step': span_ms, 'host_enqueue_ms_per_step': 1e3 * t_enq / steps,
            'steps_timed': steps, 'build_seconds': build_s, 't_1gpu_ms': ms_1gpu,
            'projected_ceiling_8gpu': ms_1gpu / t_share, 'projected_ceiling_8gpu_from_event_span': ms_1gpu / span_ms,
            'note': 'ceiling of the strong-scaling speed-up at %d GPUs with ZERO exposed communication; a measured SCALE run can only be below it' % world}


def class_api_leg(torch, data, args, engine_ms):
    """The same training step through the reference's class surface: LightGCN(args, DataLoader).train(Epoch=1) on the same graph
    (recommender/LightGCN.py:17-80), array-native DataLoader, the drop-in sampler drawing the epoch from Python's RNG, the fused engine
    behind train().  Timed: the batch loop of the epoch (first `api_steps` batches), wall clock between device synchronisations."""
    import io, contextlib, random
    from types import SimpleNamespace
    from arlib_amd.util.DataLoader import DataLoader
    from arlib_amd.recommender.LightGCN import LightGCN
    t0 = time.perf_counter()
    p = data.pairs0
    # train() evaluates on data.test_set every evalNum epochs (LightGCN.py:71-72; an empty split divides by zero there): a 1 024-row split
    ts = p[:: max(1, len(p) // 1024)][:1024]
    dl = DataLoader.from_arrays((p[:, 0], p[:, 1], np.ones(len(p), np.float32)), test=(ts[:, 0], ts[:, 1], np.ones(len(ts), np.float32)), dataName='SYN-v1')
    build_s = time.perf_counter() - t0
    a = SimpleNamespace(dataset='SYN-v1', model_name='LightGCN', maxEpoch=1, batch_size=args.batch, emb_size=args.emb, n_layers=args.layers, reg=1e-4,
                        lRate=0.005, seed=args.seed, topK='50')
    random.seed(args.seed); torch.manual_seed(args.seed)
    t1 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):          # the classes print like the reference does; stdout is the JSON line's
        rec = LightGCN(a, dl)
    init_s = time.perf_counter() - t1
    with contextlib.redirect_stdout(io.StringIO()):
        rec.max_steps_per_epoch = 20
        rec.train(Epoch=1, evalNum=1)                       # warm-up: plan build, first launches
        rec.max_steps_per_epoch = args.api_steps
        t2 = time.perf_counter()
        rec.train(Epoch=1, evalNum=1)
        epoch_wall = time.perf_counter() - t2
    st = rec.last_train_stats
    ms = 1e3 * st['loop_seconds'] / max(1, st['steps'])
    # End-to-end epoch figure, sampler INSIDE the clock (reference step = sampler + forward/backward/Adam, recommender/LightGCN.py:47-64): the epoch's
    # serial sampler part (in-place shuffle + first chunk of negatives, measured) + every batch at the measured loop pace -- the loop's clock holds whatever
    # time the steps waited for the producer thread that draws the later chunks behind the GPU (util/sampler.device_epoch)
    n_epoch = -(-len(p) // args.batch)
    epoch_s = st['first_batch_seconds'] + n_epoch * st['loop_seconds'] / max(1, st['steps'])
    return {'what': 'LightGCN(args, DataLoader.from_arrays(...)).train(Epoch=1) on the same cfg2 graph, first %d batches of the epoch' % st['steps'],
            'ms_per_step': ms, 'value': args.batch * st['steps'] / st['loop_seconds'], 'unit': 'interactions/s', 'steps': st['steps'], 'fused_engine': st['fused'],
            'engine_step_ms': engine_ms, 'gap_vs_engine_step': ms / engine_ms - 1.0,
            'dataloader_build_seconds': build_s, 'model_init_seconds': init_s,
            'epoch_wall_interactions_per_s': len(p) / epoch_s,
            'epoch_wall': {'seconds_per_epoch': epoch_s, 'batches_per_epoch': n_epoch, 'serial_sampler_seconds': st['first_batch_seconds'],
                           'producer_thread_seconds_whole_epoch': st.get('sampler_producer_seconds'), 'chunks': st.get('sampler_chunks'),
                           'how': 'serial_sampler_seconds (measured: epoch shuffle + first chunk) + batches_per_epoch x measured loop pace over %d steps; the '
                                  'negatives of later chunks are drawn by one host thread while the GPU steps run (the loop pace includes any wait for it)' % st['steps']},
            'train_call_wall_seconds': epoch_wall, 'note': 'train() wall also holds the epoch shuffle, the wait for the producer to finish the WHOLE epoch\'s negatives '
                                                           '(the loop stops after %d of %d batches) and the epoch-end full forward' % (st['steps'], n_epoch)}


def self_launch(n, result_out):
    """Run `python -m torch.distributed.run --nnodes=1 --nproc-per-node n bench.py <same argv>` as a child and return its exit code.  The rendezvous
    is 127.0.0.1 on a free port.  stdout of the children is the saved descriptor (one JSON line from rank 0)."""
    import socket
    import subprocess
    with socket.socket() as s_:
        s_.bind(('127.0.0.1', 0))
        port = s_.getsockname()[1]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n), '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    result_out.flush()
    p = subprocess.Popen(cmd, stdout=result_out.fileno(), env=env)
    try:
        return p.wait()
    except KeyboardInterrupt:
        p.terminate()
        return p.wait()


def comm_evidence(torch, dist, backend, world, rank, dev, eng):
    """What a reader needs to answer "did RCCL see N ranks": backend as torch.distributed reports it, the RCCL version torch runs on, and per rank the
    process id, device index, device name / uuid / PCI bus id (all-gathered through the group itself)."""
    try:
        ver = '.'.join(str(x) for x in torch.cuda.nccl.version())
    except Exception as e:                                   # gloo-only builds
        ver = 'unavailable (%s)' % type(e).__name__
    pr = torch.cuda.get_device_properties(dev)
    mine = {'rank': rank, 'pid': os.getpid(), 'device_index': dev.index, 'visible_devices': torch.cuda.device_count(), 'name': pr.name,
            'uuid': str(getattr(pr, 'uuid', None)), 'pci_bus_id': getattr(pr, 'pci_bus_id', None), 'arch': getattr(pr, 'gcnArchName', None)}
    allr = [None] * world
    dist.all_gather_object(allr, mine)
    # one element per rank summed through the SAME collective the item exchange uses: world*(world+1)/2 only if every rank took part
    probe = torch.full((1,), float(rank + 1), device=dev)
    dist.all_reduce(probe)
    return {'backend': dist.get_backend(), 'is_rccl': dist.get_backend() == 'nccl', 'world_size': dist.get_world_size(), 'rccl_version': ver,
            'item_exchange': getattr(eng.comm, 'item_exchange', None), 'ranks': allr,
            'distinct_devices': len({(r['uuid'], r['pci_bus_id'], r['device_index']) for r in allr}),
            'allreduce_probe': {'sum_of_rank_plus_1': float(probe[0]), 'expected': world * (world + 1) / 2.0}}


def main():
    args = parse()
    # stdout carries exactly one line, the JSON: whatever libraries print there (RCCL's version banner at communicator start-up, the classes'
    # reference-style progress lines) is sent to stderr for the life of the process, the result is written to the saved descriptor
    sys.stdout.flush()
    result_out = os.fdopen(os.dup(1), 'w')
    os.dup2(2, 1)
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local_rank = int(os.environ.get('LOCAL_RANK', 0))
    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        # plain `python bench.py --gpus N`: start the N ranks ourselves, one process per GPU, BEFORE this process imports torch or touches the GPU
        # (children, never an exec of a GPU-initialised process); the parent only forwards the exit code.  Rank 0 of the children writes the
        # JSON line to the descriptor they inherit.
        sys.exit(self_launch(args.gpus, result_out))
    import torch
    if world != args.gpus:
        raise SystemExit('WORLD_SIZE %d != --gpus %d' % (world, args.gpus))
    # test hook (1-GPU boxes): ARL_BENCH_BACKEND=gloo + ARL_BENCH_SINGLE_DEVICE=1 runs the N>1 code path with every rank on cuda:0
    backend = os.environ.get('ARL_BENCH_BACKEND', 'nccl')
    if os.environ.get('ARL_BENCH_SINGLE_DEVICE') == '1':
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device('cuda', local_rank)
    # test hook: ARL_BENCH_FORCE_SHARDED=1 at N=1 runs the sharded engine over a 1-rank RCCL group (exercises the real backend)
    sharded = world > 1 or os.environ.get('ARL_BENCH_FORCE_SHARDED') == '1'
    if sharded:
        import torch.distributed as dist
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29517')
        os.environ.setdefault('RANK', '0')
        os.environ.setdefault('WORLD_SIZE', '1')
        if backend == 'nccl':
            dist.init_process_group('nccl', device_id=dev)       # RCCL over xGMI
        else:
            dist.init_process_group(backend)

    from arlib_amd import ops, engine
    from arlib_amd.util import synthetic
    from arlib_amd.util.sampler import MTState

    # ---------------- workload: SYN-v1 graph, xavier tables, bit-exact batches
    t_setup = time.perf_counter()
    data = synthetic.syn_v1(args.users, args.items, args.mean_deg, args.seed)
    U, I, nnz = data.training_size()
    N, d, L, B = U + I, args.emb, args.layers, args.batch
    rowptr, col = data.adjacency_pattern()
    torch.manual_seed(args.seed)                      # recommender/LightGCN.py:222-228: xavier_uniform_, user table first
    E0 = torch.cat([torch.nn.init.xavier_uniform_(torch.empty(U, d)), torch.nn.init.xavier_uniform_(torch.empty(I, d))], 0)
    mt = MTState.from_seed(args.seed)
    sampler = data.pair_sampler
    n_batches = args.warmup + args.steps
    t_s = time.perf_counter()
    sampler.shuffle(mt)
    host_batches = torch.empty(n_batches, 3, B, dtype=torch.int32).pin_memory()
    hb = host_batches.numpy()
    for k in range(n_batches):
        sampler.batch(mt, k * B, B, out=hb[k])
    t_sampler = time.perf_counter() - t_s
    dev_batches = host_batches.to(dev, non_blocking=True)
    assert int(dev_batches[:, 0].max()) < U and int(dev_batches[:, 1:].max()) < I and int(dev_batches.min()) >= 0

    if not sharded:
        w = torch.ones(2 * nnz, dtype=torch.float32, device=dev)
        col_d = torch.from_numpy(col).to(dev)
        val, _ = ops.norm_adj_values(torch.from_numpy(rowptr.astype(np.int32)).to(dev), col_d, w, N)
        del w
        A = ops.CSRGraph(rowptr, col_d, val, dev, chunk=args.chunk, validate=True)
        eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, dev, table=E0.to(dev), schedule=args.schedule)
        dev_rows = torch.cat([dev_batches[:, 0], dev_batches[:, 1] + U, dev_batches[:, 2] + U], 1).contiguous()     # packed row ids [u, U+p, U+n]
        if args.dense_step:
            step = lambda k: eng.step_dense(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2])
        else:
            step = lambda k: eng.step(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2], rows=dev_rows[k])
        barrier = lambda: None
        parallelism = 'single'
    else:
        from arlib_amd import dist_engine
        eng = dist_engine.ShardedPropagationEngine.from_pairs(data.pairs0, U, I, d, L, 1e-4, 0.005, dev, rank, world, table=E0, chunk=args.chunk,
                                                               schedule=args.schedule)
        step = (lambda k: eng.step(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2])) if args.dense_step else \
               (lambda k: eng.step_sparse(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2]))
        import torch.distributed as dist
        barrier = dist.barrier
        parallelism = 'user-sharded x%d, item partial sums all-reduced (%s) per hop' % (world, 'RCCL' if dist.get_backend() == 'nccl' else dist.get_backend())
    setup_s = time.perf_counter() - t_setup

    ev = SpmmEvents(torch)
    if not args.no_kernel_events:
        ops.EVENT_HOOK = ev

    for k in range(args.warmup):
        step(k)
    if not args.no_kernel_events and args.warmup > 0:
        ev.prepare(2 * (ev.calls_seen // args.warmup + 1) * args.steps)
    barrier(); torch.cuda.synchronize()
    ev.on = True
    t0 = time.perf_counter()
    for k in range(args.warmup, n_batches):
        lo = step(k)
    torch.cuda.synchronize(); barrier()
    dt = time.perf_counter() - t0
    ev.on = False
    ops.EVENT_HOOK = None
    loss = float(lo[0] + lo[1])
    dumped = None
    if args.dump_outputs:
        # the state after the last step of the region `ms_per_step` times (the regions below train on): copied outside every clock
        outs = capture_outputs(torch, eng, lo, U, I, d, args.seed, sharded)
        if rank == 0:
            dumped = {'dir': args.dump_outputs, 'arrays': write_outputs(args.dump_outputs, outs), 'after_steps': n_batches,
                      'rows': 'user_emb / item_emb: %d of %d user rows and %d of %d item rows of the table (sorted; seeded sample when the table exceeds %d bytes)'
                              % (outs['user_emb'].shape[0], U, outs['item_emb'].shape[0], I, DUMP_BYTES)}
        del outs
    comm_diag = comm_info = None
    if sharded:
        # diagnostic region (not part of any reported time): the same steps with an event pair around every wait on a collective -- per rank,
        # how long the compute stream stood still for communication in one step
        eng.comm.measure = True
        eng.comm.waits = []
        nd = min(args.steps, 10)
        torch.cuda.synchronize(); barrier()
        td = time.perf_counter()
        for k in range(args.warmup, args.warmup + nd):
            step(k)
        torch.cuda.synchronize()
        td = time.perf_counter() - td
        ex_ms, n_waits = eng.comm.exposed_ms()
        eng.comm.measure = False
        import torch.distributed as dist
        mine = {'rank': rank, 'exposed_comm_ms_per_step': ex_ms / nd, 'waits_per_step': n_waits / nd, 'ms_per_step_in_this_region': 1e3 * td / nd}
        allr = [None] * world
        dist.all_gather_object(allr, mine)
        comm_diag = allr
        comm_info = comm_evidence(torch, dist, backend, world, rank, dev, eng)
    # further timed regions of the same K steps (same batches again: the step's cost does not depend on the table values), each bracketed
    # like the first; `value` stays the first region (the contract), the list shows how repeatable it is
    region_s = [dt]
    for _ in range(max(0, args.repeats - 1)):
        barrier(); torch.cuda.synchronize()
        t0r = time.perf_counter()
        for k in range(args.warmup, n_batches):
            step(k)
        torch.cuda.synchronize(); barrier()
        region_s.append(time.perf_counter() - t0r)
    if sharded:
        import torch.distributed as dist
        tmax = torch.tensor(region_s, dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        region_s = [float(x) for x in tmax.tolist()]
        dt = region_s[0]

    if rank == 0:
        ms = 1e3 * dt / args.steps
        E = 2 * nnz
        step_bytes = L * (16 * E + 8 * N + 24 * N * d) + 28 * N * d + 24 * B * d
        spmm_bytes = 8 * E + 4 * (N + 1) + 8 * N * d                                        # SURVEY 8d S_spmm
        evs = ev.summary()
        res = {
            'metric': 'BPR-train interactions/sec (LightGCN d=%d L=%d + BPR + Adam, B=%d)' % (d, L, B),
            'value': B * args.steps / dt, 'unit': 'interactions/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': ms, 'higher_is_better': True, 'scaling': 'strong', 'vs_baseline': None, 'dtype': 'f32', 'data': 'synthetic',
            'config': {'workload': 'cfg2: LightGCN d=%d L=%d + BPR/L2 + dense Adam, SYN-v1 %d users x %d items, nnz=%d, B=%d, seed %d'
                                   % (d, L, U, I, nnz, B, args.seed), 'parallelism': parallelism, 'chunk': args.chunk},
            'final_loss': loss,
            'repeat_ms_per_step': {'regions': [1e3 * x / args.steps for x in region_s], 'median': 1e3 * float(np.median(region_s)) / args.steps,
                                   'spread': 1e3 * (max(region_s) - min(region_s)) / args.steps, 'note': '`value` / `ms_per_step` = the first region'},
            'step_roofline': {'bound': 'hbm', 'algorithmic_bytes_per_step': step_bytes, 'achieved': step_bytes / (ms * 1e-3) / 1e9 / world,
                              'peak': HBM_PEAK_GBS, 'unit': 'GB/s', 'frac': step_bytes / (ms * 1e-3) / 1e9 / world / HBM_PEAK_GBS,
                              'note': 'whole step, per GPU'},
            'sampler': {'host_seconds_for_%d_batches_incl_epoch_shuffle' % n_batches: t_sampler},
            'setup_seconds': setup_s,
        }
        if evs:
            # dominant kernel: the full-graph hop (spmm_blocked64_kernel x2 + split-row combine), one event pair per C-ABI SpMM call
            # full-graph launches only (the row-subset and flag-masked hops are separate, much shorter kernels)
            allv = [s.elapsed_time(e) for tag, s, e in ev.recs if tag in ('axpby', 'layersum', 'adam')]
            avg_ms = float(np.mean(allv))
            # under sharding a launch covers this rank's rows only; report the single-GPU figure only for N=1
            traffic, traffic_src = None, None
            try:        # HBM-side traffic per launch from the committed PMC passes (profiles/), only for the workload they were taken on
                traffic_src = 'profiles/' + (TRAFFIC_BLOCKED if (not sharded and A.blocked is not None) else TRAFFIC_CSR)
                pm = json.load(open(os.path.join(ROOT, traffic_src)))
                if (U, I, d, args.mean_deg, args.seed, args.chunk) == (1_000_000, 100_000, 64, 32.0, 2018, 512):
                    traffic = pm['traffic_corrected_bytes']
            except Exception:
                traffic = None
            if not sharded:
                # per variant: the plain hop moves S_spmm = 8E + 4(N+1) + 8Nd algorithmic bytes; the Adam-epilogue hop reads the operand
                # and rewrites p, m, v instead of writing Y: 8E + 4(N+1) + 4Nd + 24Nd
                var_bytes = {'axpby': spmm_bytes, 'layersum': spmm_bytes + 8 * N * d, 'adam': 8 * E + 4 * (N + 1) + 28 * N * d}
                per_variant = {k: {'ms': v[0], 'launches': v[1], 'algorithmic_bytes': var_bytes[k], 'GB/s': var_bytes[k] / (v[0] * 1e-3) / 1e9,
                                   'frac': var_bytes[k] / (v[0] * 1e-3) / 1e9 / HBM_PEAK_GBS} for k, v in evs.items() if k in var_bytes}
                attain = None
                if A.blocked is not None and args.l2_ceiling:
                    ceil_ms = l2_ceiling(torch, ops, rowptr, col, U, d, dev, args.chunk)
                    plain_ms = evs['axpby'][0] if 'axpby' in evs else avg_ms
                    attain = {'ms': ceil_ms, 'GB/s': spmm_bytes / (ceil_ms * 1e-3) / 1e9, 'frac_of_peak': spmm_bytes / (ceil_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                              'plain_hop_ms': plain_ms, 'source': 'L2-resident gather of this plan (columns & 8191: every 256-B row gather an L2 hit), measured in this run',
                              'note': 'one fp32 row gather per edge is bounded by the L2->CU gather rate (MI355X_MICROARCH.md, Indexed rows: 66-73 GB/s per CU), '
                                      'not by HBM: E x 4d bytes through the vector L1 per hop'}
                res['roofline'] = {'bound': 'hbm', 'achieved': spmm_bytes / (avg_ms * 1e-3) / 1e9, 'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                                   'frac': spmm_bytes / (avg_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 'traffic': traffic,
                                   'attainable': attain, 'frac_of_attainable': (attain['ms'] / attain['plain_hop_ms']) if attain else None,
                                   'per_variant': per_variant,
                                   'traffic_source': (traffic_src + ' (rocprofv3 --pmc FETCH_SIZE/WRITE_SIZE pass of this workload, gfx950-corrected; NOT measured in this run)') if traffic is not None else None,
                                   'kernel': ('one full-graph hop = spmm_blocked64_kernel<%d,*> x%d (user rows, item rows; %d rows above the per-set threshold dealt as strided '
                                              'pieces + spmm_long_rows_kernel combine, %d rows on the chunked CSR kernel); avg over %d hops'
                                              % (A.blocked.rpw, len(A.blocked.sets), sum(s_['n_split'] for s_ in A.blocked.sets), A.blocked.n_hub, len(allv))) if A.blocked is not None
                                   else 'spmm_rows_kernel<LPR=%d> (+spmm_long_rows_kernel), avg over %d launches' % (max(4, d // 4), len(allv)),
                                   'schedule': 'blocked' if A.blocked is not None else 'csr',
                                   'avg_launch_ms': avg_ms, 'algorithmic_bytes_per_launch': spmm_bytes,
                                   'per_variant_ms': {k: v[0] for k, v in evs.items()},
                                   'gather_model_bytes_per_launch': E * (8 + 4 * d) + 4 * N * d,
                                   # ceilings from the chip's own figures (MI355X_MICROARCH.md), independent of this implementation: a pull SpMM moves one
                                   # 4d-byte row per edge through the vector L1s whatever the HBM-side traffic
                                   'chip_ceilings': {'row_gather_bytes_per_launch': E * 4 * d,
                                                     'ms_at_L2_peak_34.5TBs': E * 4 * d / 34.5e12 * 1e3,
                                                     'ms_at_guide_L2_resident_row_gather_16.8_to_18.8TBs': [E * 4 * d / 18.8e12 * 1e3, E * 4 * d / 16.8e12 * 1e3],
                                                     'ms_for_measured_fabric_traffic_at_6.3TBs_achievable_HBM': (traffic / 6.3e12 * 1e3) if traffic else None,
                                                     'frac_of_peak_if_at_guide_gather_rate': spmm_bytes / (E * 4 * d / 16.8e12) / 1e9 / HBM_PEAK_GBS,
                                                     'note': '`attainable` above is THIS kernel with every gather an L2 hit; these are the guide\'s rates for the same bytes'}}
            else:
                res['spmm_events_ms'] = {k: v[0] for k, v in evs.items()}
        if dumped is not None:
            res['dump_outputs'] = dumped
        if comm_info is not None:
            res['comm'] = comm_info
        if comm_diag is not None:
            res['communication'] = {'per_rank': comm_diag, 'note': 'separate diagnostic region: event pairs around every wait on an all-reduce; exposed = time the '
                                    'compute stream was blocked by the collective (0 = fully hidden behind the SpMM kernels)'}
        if not sharded:
            # A/B: the reference-shaped step (all 2L hops over the full graph), same engine state, few steps
            other = (lambda k: eng.step(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2], rows=dev_rows[k])) if args.dense_step else \
                    (lambda k: eng.step_dense(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2]))
            other(0); torch.cuda.synchronize()
            t1 = time.perf_counter()
            nn = min(8, n_batches)
            for k in range(nn):
                other(k)
            torch.cuda.synchronize()
            res['ab_compare'] = {'main_step': 'dense (2L full hops)' if args.dense_step else 'sparse-batch (2L-2 full hops + row-subset + flag-masked hop)',
                                 'other_step_ms': 1e3 * (time.perf_counter() - t1) / nn}
        if not sharded and args.attack_steps > 0:
            E0_snapshot = eng.E0.clone()
            del eng.Ea, eng.Eb, eng.S
            res['attack'] = attack_leg(torch, ops, data, E0_snapshot, args)
            torch.cuda.empty_cache()
            res['attack_clear'] = clear_leg(torch, ops, data, eng.A, E0_snapshot, args)
            # DLAttack's inner step (attack/White/DLAttack.py:86-113) is the BPR/Adam step of the headline metric on the
            # surrogate (its CW term is a detached constant); the scoring pass above runs once per outer epoch
            res['attack_dlattack_inner'] = {'value': 1e3 / ms, 'unit': 'steps/s', 'note': 'same fused step as `value` (B=%d)' % B}
        if not sharded and args.attack_steps > 0 and d in (16, 32, 64, 128):
            torch.cuda.empty_cache()
            res['ncl_structure_term'] = ncl_structure_leg(torch, E0_snapshot, args)
        if not sharded and args.model_steps > 0 and args.emb in (64, 128):
            E0_snapshot = None
            torch.cuda.empty_cache()
            res.update(model_legs(torch, ops, engine, data, eng.A, dev_batches, args, steps=args.model_steps))
        if not sharded and args.share_steps > 0 and U >= 8 * 64:
            torch.cuda.empty_cache()
            sh = share_leg(torch, data, E0, dev_batches, args, float(np.median(region_s)) * 1e3 / args.steps, steps=args.share_steps)
            res['rank_share_n8'] = sh
            res['projected_ceiling_8gpu'] = sh['projected_ceiling_8gpu']
        if not sharded and args.api_steps > 0:
            torch.cuda.empty_cache()
            res['class_api'] = class_api_leg(torch, data, args, float(np.median(region_s)) * 1e3 / args.steps)
        if not sharded and args.cpu_baseline:
            val_np = eng.A.val.cpu().numpy()
            batches = [(hb[k, 0].copy(), hb[k, 1].copy(), hb[k, 2].copy()) for k in range(min(n_batches, 8))]
            def gpu_replay(k_steps):
                e2 = engine.PropagationEngine(eng.A, U, I, d, L, 1e-4, 0.005, dev, table=E0.to(dev))
                for k in range(k_steps):
                    e2.step(dev_batches[k, 0], dev_batches[k, 1], dev_batches[k, 2])
                return e2.E0.cpu().numpy()
            res['cpu_baseline'] = cpu_baseline(data, rowptr, col, val_np, E0.numpy(), batches, args, args.cpu_seconds, gpu_replay)
            if args.cpu_torch > 0:
                res['cpu_baseline_torch'] = cpu_torch_baseline(torch, rowptr, col, val_np, E0, batches, U, args, min(args.cpu_torch + 1, len(batches)))
        result_out.write(json.dumps(res) + '\n')
        result_out.flush()
    if sharded:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == '__main__':
    main()

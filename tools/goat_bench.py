#!/usr/bin/env python3
"""GOAT's pieces at cfg2's graph (SYN-v1, 1 M users x 100 K items), the co-rating kernel against scipy at instance M (100 K x 20 K), and the whole
default attack on ml-100k.  Prints one JSON line and writes it to profiles/goat_bench.json.

    python tools/goat_bench.py [--users 1000000 --items 100000 --reps 5] [--scipy-limit 240] [--reference-seconds S] [--skip-default]

cfg2 (F = 1 % of the users, k = int(nnz / U), 5 targets):
  corating_kernel_ms     arl_corating_degree_i32 alone (device events, median of --reps), on an item-major index and launch order that exist already;
  corating_call_ms       one corating.corating_degree call: the index, the order, the kernel;
  item_sample_ms         one itemSample call in the library on data validated once, as the attack calls it (host clock, median);
  item_sample_with_validation_ms   the same through a fresh SampleData, i.e. with the range checks of the CSR in every call;
  d_step_ms, g_step_ms   one D and one G step (torch autograd on the device, util.optim.Adam; device events);
  generate_ms            the final generation: G's forward and the row-chunked projection (host clock around a call that ends in a host read).
instance M: corating.corating_degree against corating.corating_degree_host in a child process that never opens the GPU, under --scipy-limit
  seconds; a run that did not finish is reported as such with the limit as the lower bound of its time.
ml-100k: GOAT(arg, data).posionDataAttack() with the reference's defaults (50 x (20 + 20) steps, 2 001 itemSample calls), host clock;
  --reference-seconds records the reference's own CPU run of the same call, taken where the reference is at hand, and --reference-host where and
  how that was (another machine's CPU: the two times are stated side by side, no ratio is formed)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                            # noqa: E402
import scipy.sparse as sp                     # noqa: E402


def graph(U, I, seed=2018):
    from arlib_amd.util import synthetic
    p = synthetic.syn_v1_pairs_native(U, I, 32.0, seed)
    X = sp.csr_matrix((np.ones(len(p), np.float32), (p[:, 0], p[:, 1])), shape=(U, I))
    X.sort_indices()
    return X


def host_child(U, I):
    from arlib_amd import corating
    X = graph(U, I)
    t = time.perf_counter()
    out = corating.corating_degree_host(X)
    print(json.dumps(dict(seconds=time.perf_counter() - t, checksum=float(out.sum()))), flush=True)


def events_ms(fn, reps):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def host_ms(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1_000_000)
    ap.add_argument('--items', type=int, default=100_000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scipy-limit', type=float, default=240.0)
    ap.add_argument('--reference-seconds', type=float, default=None)
    ap.add_argument('--reference-host', default=None, help='where and how --reference-seconds was taken (recorded beside it)')
    ap.add_argument('--skip-default', action='store_true')
    ap.add_argument('--host-child', type=int, nargs=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.host_child:
        return host_child(*a.host_child)

    import random
    import torch
    from arlib_amd import corating, _lib, ops
    from arlib_amd.attack.Gray import GOAT as M
    from arlib_amd.util.optim import Adam
    if not torch.cuda.is_available():
        sys.exit('goat_bench: needs a GPU (a time taken anywhere else says nothing)')
    out = {}

    # ---- cfg2
    U, I = a.users, a.items
    X = graph(U, I)
    F, k, targets = int(U * 0.01), int(X.nnz / U), [11, 222, 3333, 44444 % I, I - 1]
    rp, ci = torch.from_numpy(X.indptr.astype(np.int64)).cuda(), torch.from_numpy(X.indices.astype(np.int32)).cuda()
    deg_u = np.diff(X.indptr).astype(np.float64)
    t_call = events_ms(lambda: corating.corating_degree(rp, ci, U, I), a.reps)
    cnt = corating.corating_degree(rp, ci, U, I)
    # the kernel alone, on the index corating_degree builds
    i_colptr, i_row, order = corating._item_major(rp, ci, U, I)
    res = torch.empty(I, dtype=torch.int32, device='cuda')
    L, P = _lib.lib(), ops._ptr

    def kernel(order_t):
        _lib.check(L.arl_corating_degree_i32(P(rp), P(ci), P(i_colptr), P(i_row), U, I, P(order_t), P(res), ops._stream()), 'arl_corating_degree_i32')
    t_kernel = events_ms(lambda: kernel(order), a.reps)
    assert torch.equal(res, cnt)
    t_plain = events_ms(lambda: kernel(None), a.reps)
    ors = float((deg_u ** 2).sum())
    out['cfg2'] = dict(users=U, items=I, nnz=int(X.nnz), fake_users=F, k=k, lds_bit_ors=ors,
                       corating_kernel_ms=t_kernel[0], corating_kernel_ms_min_max=t_kernel[1:], corating_kernel_index_order_ms=t_plain[0],
                       corating_kernel_gors_per_s=ors / t_kernel[0] / 1e6, corating_call_ms=t_call[0], corating_call_ms_min_max=t_call[1:],
                       degree_min_max=[int(cnt.min()), int(cnt.max())])
    cnt_h = cnt.cpu().numpy().astype(np.float64)
    random.seed(11)
    torch.manual_seed(11)
    data = M.SampleData(X.indptr, X.indices, U, I, cnt_h, targets)                 # validated once, as GOAT's constructor does
    sample = lambda: M.item_sample(data, F, k, 0.01, 0.02)
    assert M.native_sampling_exact(k, len(targets), I)
    t_sample = host_ms(sample, a.reps)
    t_sample_v = host_ms(lambda: M.item_sample(M.SampleData(X.indptr, X.indices, U, I, cnt_h, targets), F, k, 0.01, 0.02), a.reps)
    I_s, I_f, real, user = sample()
    G, D = M.Encoder(k).cuda(), M.Decoder(k).cuda()
    opt_G, opt_D = Adam(G.parameters(), lr=0.005), Adam(D.parameters(), lr=0.005)
    Z, realt = torch.randn(F, k).cuda(), torch.from_numpy(real).cuda().float()
    t_d = events_ms(lambda: M.d_step(G, D, opt_D, Z, realt), a.reps)
    t_g = events_ms(lambda: M.g_step(G, D, opt_G, Z, realt, k), a.reps)

    def generate():
        with torch.no_grad():
            return M.project_rows(G(Z), I_s, I_f, targets, I, k)
    t_gen = host_ms(generate, max(2, a.reps // 2))
    out['cfg2'].update(users_with_min_items=int((deg_u >= 0.01 * I).sum()), item_sample_ms=t_sample[0], item_sample_ms_min_max=t_sample[1:],
                       real_user_items=int(deg_u[user]), item_sample_with_validation_ms=t_sample_v[0], d_step_ms=t_d[0], d_step_ms_min_max=t_d[1:], g_step_ms=t_g[0], g_step_ms_min_max=t_g[1:],
                       generate_ms=t_gen[0], generate_ms_min_max=t_gen[1:])
    del X, rp, ci, i_row, i_colptr, order, res, G, D, Z, realt
    torch.cuda.empty_cache()

    # ---- instance M against scipy
    Um, Im = 100_000, 20_000
    Xm = graph(Um, Im)
    rpm, cim = torch.from_numpy(Xm.indptr.astype(np.int64)).cuda(), torch.from_numpy(Xm.indices.astype(np.int32)).cuda()
    t_m = events_ms(lambda: corating.corating_degree(rpm, cim, Um, Im), a.reps)
    dev_sum = float(corating.corating_degree(rpm, cim, Um, Im).sum())
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), '--host-child', str(Um), str(Im)], stdout=subprocess.PIPE, text=True,
                             env=dict(os.environ, HIP_VISIBLE_DEVICES=''))
    try:
        text, finished = child.communicate(timeout=a.scipy_limit)[0], True
    except subprocess.TimeoutExpired:
        child.kill()
        text, finished = child.communicate()[0], False
    host = [json.loads(line) for line in text.splitlines() if line.startswith('{')]
    m = dict(users=Um, items=Im, nnz=int(Xm.nnz), corating_call_ms=t_m[0], corating_call_ms_min_max=t_m[1:], scipy_limit_s=a.scipy_limit,
             scipy_finished=bool(finished and host))
    if host:
        m.update(scipy_s=host[0]['seconds'], same_result=host[0]['checksum'] == dev_sum, scipy_over_device=host[0]['seconds'] * 1e3 / t_m[0])
    else:
        m.update(scipy_over_device_at_least=a.scipy_limit * 1e3 / t_m[0])
    out['instance_M'] = m

    # ---- the default attack on ml-100k
    if not a.skip_default:
        from arlib_amd.util.DataLoader import DataLoader
        from arlib_amd.util.tool import seedSet
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'ml100k_data.npz'))
        seedSet(2018)
        data = DataLoader.from_arrays((g['train_u'], g['train_i'], g['train_r']), (g['val_u'], g['val_i'], g['val_r']), (g['test_u'], g['test_i'], g['test_r']),
                                      dataName='ml-100k')
        arg = SimpleNamespace(maliciousUserSize=0.01, maliciousFeedbackSize=0, Epoch=1, innerEpoch=1, outerEpoch=1, attackTargetChooseWay='unpopular', targetSize=5)
        torch.cuda.synchronize()
        t = time.perf_counter()
        atk = M.GOAT(arg, data)
        torch.cuda.synchronize()
        t_ctor = time.perf_counter() - t
        random.seed(11); np.random.seed(11); torch.manual_seed(11)
        t = time.perf_counter()
        res = atk.posionDataAttack()
        torch.cuda.synchronize()
        t_attack = time.perf_counter() - t
        d = dict(users=atk.userNum, items=atk.itemNum, fake_users=atk.fakeUserNum, k=atk.k, steps=len(atk.loss_log), item_sample_calls=len(atk.real_users),
                 constructor_s=t_ctor, attack_s=t_attack, fake_rows=int(res.shape[0] - atk.userNum))
        if a.reference_seconds is not None:
            d.update(reference_cpu_attack_s=a.reference_seconds, reference_cpu_attack_taken=a.reference_host or 'not recorded')
        out['ml100k_default'] = d
    line = json.dumps(out)
    print(line)
    with open(os.path.join(ROOT, 'profiles', 'goat_bench.json'), 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()

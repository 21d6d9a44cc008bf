#!/usr/bin/env python3
"""AUSH's GAN at cfg2 size (I = 100 K items -> S = I // 5 + 5 = 20 005, F = 10 000 fake users): the template build (both mask sources), one
D step, one G step and the final generation, fused (arl_gan_* kernels) against the composed torch route (torch.sparse.mm + F.linear + autograd)
on the same device; both routes step with the same Adam.  Prints one JSON line: ms per phase (median of --reps after a warm-up), the
TFLOP/s of the G step's three F x S x S products and their fraction of the 157 TFLOP/s fp32 matrix peak.

    python tools/aush_bench.py [--users 1000000] [--items 100000] [--reps 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from arlib_amd import ops                                       # noqa: E402
from arlib_amd.attack.Gray import _gan                          # noqa: E402
from arlib_amd.attack.Gray.AUSH import Generator, Discriminator, draw_masks  # noqa: E402
from arlib_amd.util.optim import Adam                           # noqa: E402

PEAK_TFLOPS = 157.0


def timed(fn, reps, warm=True):
    if warm:
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1000000)
    ap.add_argument('--items', type=int, default=100000)
    ap.add_argument('--per-user', type=int, default=60)
    ap.add_argument('--reps', type=int, default=3)
    a = ap.parse_args()
    U, I, T = a.users, a.items, 5
    F, S = U // 100, I // 5 + T
    rng = np.random.default_rng(0)
    nnz = U * a.per_user
    u = np.repeat(np.arange(U), a.per_user)
    it = np.minimum((rng.pareto(1.2, nnz) * 50).astype(np.int64), I - 1)
    ui = sp.csr_matrix((np.ones(nnz, np.float32), (u, it)), shape=(U, I), dtype=np.float32)
    ui.data[:] = 1.0
    ui.sort_indices()
    itemP = np.asarray(ui.sum(0) / ui.sum()).ravel().astype(np.float32)
    targets = rng.choice(I, T, replace=False)
    itemP[targets] = 0
    pool = np.setdiff1d(np.arange(I), targets)
    select = np.concatenate([rng.choice(pool, I // 5, replace=False), targets])
    pos = np.full(I, -1, np.int32)
    pos[select] = np.arange(S)
    d = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    rowptr, col, val = d(ui.indptr, np.int64), d(ui.indices, np.int32), d(ui.data, np.float32)
    pos_d, items_d, ip_d = d(pos, np.int32), d(select, np.int32), d(itemP, np.float32)
    users = d(rng.choice(U, F, replace=False), np.int32)
    out = dict(F=F, S=S, I=I, U=U)

    itemP64 = itemP.astype(np.float64)
    np.random.seed(0)

    def host_template():                                                # the default source as AUSH._template runs it: draw_masks + the kernel
        m = torch.from_numpy(draw_masks(itemP64, select, F)).cuda()
        return _gan.Template(*ops.gan_template(users, rowptr, col, val, pos_d, items_d, mask=m), S)
    out['template_host_ms'] = timed(host_template, 1, warm=False)
    out['template_device_ms'] = timed(lambda: _gan.Template(*ops.gan_template(users, rowptr, col, val, pos_d, items_d, item_p=ip_d, seed=1, call=0), S), a.reps)
    tpl = _gan.Template(*ops.gan_template(users, rowptr, col, val, pos_d, items_d, item_p=ip_d, seed=1, call=0), S)
    out['template_nnz'] = int(tpl.col.numel())
    torch.manual_seed(0)
    G, D = Generator(S).cuda(), Discriminator(S).cuda()
    oG, oD = Adam(G.parameters(), lr=0.005), Adam(D.parameters(), lr=0.005)
    for tag, fused in (('fused', True), ('composed', False)):
        out[tag + '_d_step_ms'] = timed(lambda: _gan.d_step(G, D, oD, tpl, T, fused), a.reps)
        out[tag + '_g_step_ms'] = timed(lambda: _gan.g_step(G, D, oG, tpl, T, fused), a.reps)
        out[tag + '_generate_ms'] = timed(lambda: _gan.generate(G, tpl, fused), a.reps)
    # the fused G step piece by piece (each piece timed alone, synchronised): where its time goes outside the three products
    W1, b1, W2, b2, wD, bD = _gan._params(G, D)
    st = {}
    st['W1t'] = ops.gan_transpose(W1.detach())
    st['H'] = ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, st['W1t'], bias=b1.detach(), relu=True, check_range=False)
    st['Y'] = ops.gan_gemm(st['H'], W2.detach(), trans_b=True, epilogue=ops.GAN_EPI_BIAS_SIGMOID, bias=b2.detach())
    st['rows'] = ops.gan_rows(st['Y'], tpl.Td, T, wD.detach(), bD.detach())
    st['dZ2'] = ops.gan_dz2(st['Y'], tpl.Td, st['rows'][0], st['rows'][3], wD.detach(), T)
    st['dZ1'] = ops.gan_gemm(st['dZ2'], W2.detach(), epilogue=ops.GAN_EPI_RELU_MASK, aux=st['H'])
    st['dW1t'] = ops.gan_spmm(tpl.csc_ptr, tpl.csc_row, tpl.csc_val, st['dZ1'], check_range=False)
    parts = {
        'transpose_W1': lambda: ops.gan_transpose(W1.detach()),
        'layer1_spmm': lambda: ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, st['W1t'], bias=b1.detach(), relu=True, check_range=False),
        'layer2_gemm': lambda: ops.gan_gemm(st['H'], W2.detach(), trans_b=True, epilogue=ops.GAN_EPI_BIAS_SIGMOID, bias=b2.detach()),
        'rows_losses': lambda: ops.gan_rows(st['Y'], tpl.Td, T, wD.detach(), bD.detach()),
        'dz2': lambda: ops.gan_dz2(st['Y'], tpl.Td, st['rows'][0], st['rows'][3], wD.detach(), T),
        'dW2_gemm': lambda: ops.gan_gemm(st['dZ2'], st['H'], trans_a=True),
        'db2_colsum': lambda: ops.gan_colsum(st['dZ2']),
        'dH_gemm': lambda: ops.gan_gemm(st['dZ2'], W2.detach(), epilogue=ops.GAN_EPI_RELU_MASK, aux=st['H']),
        'db1_colsum': lambda: ops.gan_colsum(st['dZ1']),
        'dW1t_spmm_csc': lambda: ops.gan_spmm(tpl.csc_ptr, tpl.csc_row, tpl.csc_val, st['dZ1'], check_range=False),
        'transpose_dW1': lambda: ops.gan_transpose(st['dW1t']),
        'adam_G': lambda: oG.step(),
    }
    out['fused_g_step_parts_ms'] = {k: round(timed(f, a.reps), 3) for k, f in parts.items()}
    out['template_max_col_nnz'] = int((tpl.csc_ptr[1:] - tpl.csc_ptr[:-1]).max())
    del st
    flops = 3 * 2.0 * F * S * S
    W2 = G.net.layer_1.weight.detach()
    H = torch.rand(F, S, device='cuda')
    out['gemm_fwd_ms'] = timed(lambda: ops.gan_gemm(H, W2, trans_b=True), a.reps)
    out['gemm_dw_ms'] = timed(lambda: ops.gan_gemm(H, H, trans_a=True), a.reps)
    out['gemm_dh_ms'] = timed(lambda: ops.gan_gemm(H, W2), a.reps)
    gemm_ms = out['gemm_fwd_ms'] + out['gemm_dw_ms'] + out['gemm_dh_ms']
    out['products_tflops'] = flops / (gemm_ms * 1e-3) / 1e12
    out['products_peak_fraction'] = out['products_tflops'] / PEAK_TFLOPS
    out['g_step_bound_ms'] = flops / (PEAK_TFLOPS * 1e12) * 1e3
    out['fused_vs_composed_g_step'] = out['composed_g_step_ms'] / out['fused_g_step_ms']
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == '__main__':
    main()

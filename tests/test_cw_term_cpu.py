"""The attacks' CW term past arl_cw_topk_term_f32's limits, on CPU: ops.cw_topk_term_supported against the kernel's shape checks, and
attack._common.cw_term / cw_term_rows (the row-primitive restatement the attacks and the sharded CLeaR step fall back to) against the float64
restatement of the term in the CPU test double.  The same routes on the device are in test_gpu_attack_edges.py."""
import numpy as np
import pytest
import torch

import cpu_kernels_shim as shim
from arlib_amd import ops
from arlib_amd.attack._common import cw_term, cw_term_rows


@pytest.mark.parametrize('I,d,T,k,want', [
    (1_048_576, 64, 5, 50, True), (1_048_577, 64, 5, 50, False),            # 8 192 groups of 128 items
    (1_048_576, 128, 5, 50, True), (1_048_577, 128, 5, 50, False),
    (524_288, 132, 5, 50, True), (524_289, 132, 5, 50, False),              # d > 128: groups of 64 items
    (524_288, 256, 5, 50, True), (524_289, 256, 5, 50, False),
    (100, 64, 64, 64, True), (100, 64, 65, 80, False), (100, 64, 100, 128, False),
    (100, 64, 8, 7, False), (100, 64, 0, 7, False),
    (100, 4, 1, 1, True), (100, 260, 1, 1, False), (100, 66, 1, 1, False), (100, 0, 1, 1, False),
])
def test_cw_topk_term_supported_boundaries(I, d, T, k, want):
    assert ops.cw_topk_term_supported(I, d, T, k) is want


def _problem(seed, Up, n_real, I, d, k, targets):
    g = torch.Generator().manual_seed(seed)
    X = (torch.randn(Up + I, d, generator=g, dtype=torch.float64) * 10.0 ** torch.randint(-2, 1, (Up + I, 1), generator=g)).float()
    top = torch.stack([torch.randperm(I, generator=g)[:k] for _ in range(Up)]).to(torch.int32)
    top[: n_real // 2, k - 1] = 3                                               # a popular tail item (many addends on one row)
    return X, top, torch.tensor(targets, dtype=torch.int64)


@pytest.mark.parametrize('n_real,F,I,d,k,targets', [
    (300, 5, 400, 16, 80, list(range(0, 140, 2))),                              # T = 70 > 64
    (300, 5, 400, 12, 80, [7] * 3 + list(range(100, 167))),                     # T = 70 with a target listed three times
    (50, 3, 90, 8, 7, [1, 2, 2, 89, 0, 5, 6]),                                  # T = k, repeated target
    (0, 4, 90, 8, 10, [1, 2, 3]),                                               # no real users: loss, G and w are 0
])
def test_cw_term_rows_equals_float64_term(n_real, F, I, d, k, targets):
    """cw_term_rows against the float64 restatement (tests/cpu_kernels_shim.py): loss, G on every row, the SFA multiplicities w exactly,
    repeated targets counted once per listing; cw_term routes T > 64 there and gives the same."""
    Up = n_real + F
    X, top, tg = _problem(n_real + I + d, Up, n_real, I, d, k, targets)
    lo_ref, G_ref, w_ref = shim.cw_topk_term(X, Up, n_real, top, tg)
    lo, G, w = cw_term_rows(X, Up, n_real, top, tg, kern=shim)
    Gd = G_ref.double()
    assert abs(float(lo[0]) - float(lo_ref[0])) <= 1e-5 * max(abs(float(lo_ref[0])), float(Gd.abs().max()), 1e-30)
    assert float((G.double() - Gd).abs().max()) <= 1e-5 * max(float(Gd.abs().max()), 1e-30)
    assert torch.equal(w, w_ref)
    if n_real == 0:
        assert float(lo[0]) == 0.0 and not G.any() and not w.any()
    assert not G[n_real:Up].any() and not w[n_real:Up].any()                  # fake users take no part in the pairs
    lo2, G2, w2 = cw_term(X, Up, n_real, top, tg, kern=shim)
    if len(targets) > 64:
        assert torch.equal(lo2, lo) and torch.equal(G2, G) and torch.equal(w2, w)
    _, _, w3 = cw_term_rows(X, Up, n_real, top, tg, want_w=False, kern=shim)
    assert w3 is None


def test_cw_term_rejects_more_targets_than_list_entries():
    X, top, tg = _problem(1, 20, 20, 50, 8, 10, list(range(11)))
    with pytest.raises(ValueError):
        cw_term(X, 20, 20, top, tg, kern=shim)
    with pytest.raises(ValueError):
        cw_term_rows(X, 20, 20, top, tg, kern=shim)
    with pytest.raises(IndexError):
        bad = top.clone(); bad[0, -1] = 50
        cw_term_rows(X, 20, 20, bad, tg[:5], kern=shim)

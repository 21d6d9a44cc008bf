"""CPU tests of the rest of util.loss (alignment_loss, uniformity_loss, batch_softmax_loss, kl_divergence, js_divergence): the composed route on
float64 inputs against the reference's float64 values (g33_pairloss.npz), the C surface, and the float64 numpy restatement of the uniformity
kernel's formula that tests/test_gpu_pairloss.py measures the kernel against."""
import math
import os
import re
import numpy as np
import pytest
import torch
from conftest import golden, ROOT
from test_ncf_wrmf_cpu import pick

F64_TOL = 1e-9          # float64 routes that differ only in the order of their sums: eps 1.1e-16 times the 1e-3 cancellation of the clustered set, with room


def g33():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'g33_pairloss.npz'), allow_pickle=False)


def unif_sets(g):
    return [(str(name), int(n), int(d)) for name, (n, d) in zip(g['unif_sets'], g['unif_shapes'])]


def unif_input(g, name):
    """The float32 input of a uniformity set, rebuilt from what the fixture stores (tests/golden/gen_golden_pairloss.py)."""
    if name + '__x' in g.files:
        return g[name + '__x'].astype(np.float32)
    centres, jitter = g[name + '__centres'], g[name + '__jitter']
    x = centres[np.arange(jitter.shape[0]) % 4] + jitter.astype(np.float32)
    x[1] = x[0]
    if x.shape[0] > 3:
        x[3] = 0.0
    return x


def uniformity_restated(x, t=2.0):
    """float64 numpy restatement of arl_uniformity_fwd_bwd_f32's formula (not of torch.pdist): (loss, dloss/dx) for raw rows x."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    norm = np.sqrt((x * x).sum(1))
    nrm = np.maximum(norm, 1e-12)
    y = x / nrm[:, None]
    q = (y * y).sum(1)
    e = np.exp(-t * np.maximum(q[:, None] + q[None, :] - 2.0 * (y @ y.T), 0.0))
    e[np.arange(n), np.arange(n)] = 0.0                                     # the diagonal is masked, not subtracted
    rowsum, Gm = e.sum(1), e @ y
    S = rowsum.sum()
    loss = math.log(S / (n * (n - 1.0)))
    dy = (-4.0 * t / S) * (y * rowsum[:, None] - Gm)
    dot = np.where(norm > 1e-12, (y * dy).sum(1), 0.0)                       # a row at the clamp passes its gradient divided by the clamp
    return loss, (dy - y * dot[:, None]) / nrm[:, None]


def rel(a, b):
    den = np.linalg.norm(b)
    return np.linalg.norm(np.asarray(a, np.float64) - b) / (den if den > 0 else 1.0)


def grads(fn, *arrays):
    ts = [torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in arrays]
    loss = fn(*ts)
    return loss.item(), [t.numpy() for t in torch.autograd.grad(loss, ts)]


def test_fixture_holds_numbers_only_and_the_sets_the_tests_need():
    g = g33()
    assert all(g[k].dtype.kind in 'fiuU' for k in g.files)
    sets = unif_sets(g)
    assert [s[1:] for s in sets[:4]] == [(2, 16), (17, 16), (130, 64), (1061, 128)] and len(sets) == 10 and sets[4][1:] == sets[9][1:]
    assert [s[0].split('_')[1] for s in sets] == ['gauss'] * 5 + ['clust'] * 5
    x = unif_input(g, 'unif_clust_17x16')
    assert np.array_equal(x[0], x[1]) and not x[3].any() and x[2].any()
    g4 = np.load(os.path.join(ROOT, 'tests', 'golden', 'g34_directau.npz'), allow_pickle=False)
    assert len(g4['align_losses']) == len(g4['unif_losses']) == len(g4['batch_sizes']) == 25


def test_composed_float64_route_equals_reference_float64():
    from arlib_amd.util import loss as L
    g = g33()
    for name, n, d in unif_sets(g):
        lo, (gx,) = grads(L.uniformity_loss, unif_input(g, name))
        assert abs(lo - float(g[name + '__loss64'])) <= F64_TOL, name
        assert rel(pick(gx, g, name + '__grad64'), g[name + '__grad64']) <= F64_TOL, name
    x, y = g['align_130x64__x'], g['align_130x64__y']
    for alpha in (1, 2):
        k = 'align_130x64_a%d__' % alpha
        lo, (gx, gy) = grads(lambda a, b: L.alignment_loss(a, b, alpha), x, y)
        assert abs(lo - float(g[k + 'loss64'])) <= F64_TOL
        assert rel(pick(gx, g, k + 'gradx64'), g[k + 'gradx64']) <= F64_TOL and rel(pick(gy, g, k + 'grady64'), g[k + 'grady64']) <= F64_TOL
        r = int(g['align_130x64__same_row'])
        assert not gx[r].any() and not gy[r].any() and not g[k + 'same_row_grads'].any()
    for key, fn in (('bsm', lambda a, b: L.batch_softmax_loss(a, b, 0.2)), ('kl', L.kl_divergence), ('js', L.js_divergence)):
        lo, (ga, gb) = grads(fn, g[key + '__a'], g[key + '__b'])
        assert abs(lo - float(g[key + '__loss64'])) <= F64_TOL, key
        assert rel(ga, g[key + '__grada64']) <= F64_TOL and rel(gb, g[key + '__gradb64']) <= F64_TOL, key
        assert abs(float(g[key + '__loss32']) - lo) <= 1e-5 * max(1.0, abs(lo))


def test_reference_names_signatures_and_defaults():
    import inspect
    from arlib_amd.util import loss as L
    for name in ('bpr_loss', 'wrmf_loss', 'alignment_loss', 'uniformity_loss', 'l2_reg_loss', 'batch_softmax_loss', 'InfoNCE', 'kl_divergence', 'js_divergence'):
        assert callable(getattr(L, name)), name
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E = inspect.Parameter.empty
    assert sig(L.alignment_loss) == [('x', E), ('y', E), ('alpha', 2)] and sig(L.uniformity_loss) == [('x', E), ('t', 2)]
    assert sig(L.batch_softmax_loss) == [('user_emb', E), ('item_emb', E), ('temperature', E)]
    assert sig(L.kl_divergence) == sig(L.js_divergence) == [('p_logit', E), ('q_logit', E)]
    assert 'composed from torch ops' in L.kl_divergence.__doc__.lower() and 'composed from torch ops' in L.js_divergence.__doc__.lower()


def test_fewer_than_two_rows_give_nan_like_the_reference():
    from arlib_amd.util.loss import uniformity_loss
    assert math.isnan(uniformity_loss(torch.randn(1, 16)).item())
    assert math.isnan(uniformity_loss(torch.randn(1, 64, dtype=torch.float64)).item())


def test_header_exports_and_argument_checks():
    from arlib_amd import _lib, pairloss
    names = ('arl_uniformity_splits', 'arl_uniformity_workspace_bytes', 'arl_uniformity_fwd_bwd_f32', 'arl_alignment_fwd_bwd_f32')
    hdr = open(os.path.join(ROOT, 'include', 'arlib_amd.h')).read()
    for name in names:
        assert name in _lib.EXPORTS and re.search(r'\b%s\s*\(' % name, hdr), name
    assert 'util/loss.py:17-23' in hdr
    L = _lib.lib()
    assert L.arl_abi_version() == _lib.ABI_VERSION == 34
    assert pairloss.PAIRLOSS_WIDTHS == (16, 32, 64, 128) and pairloss.PAIRLOSS_MAX_ROWS == (2 ** 31 - 1) // 128
    # arguments are checked before any launch: no device is needed to be told so
    assert L.arl_uniformity_fwd_bwd_f32(None, 4, 16, 2.0, 1.0, None, None, None, None) == -1
    buf = np.zeros(64, np.float32)
    p = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert L.arl_uniformity_fwd_bwd_f32(p, 4, 20, 2.0, 1.0, p, None, p, None) == -2
    assert L.arl_uniformity_fwd_bwd_f32(p, 1, 16, 2.0, 1.0, p, None, p, None) == -4
    assert L.arl_uniformity_fwd_bwd_f32(p, 4, 16, 0.0, 1.0, p, None, p, None) == -4
    assert L.arl_uniformity_fwd_bwd_f32(p, pairloss.PAIRLOSS_MAX_ROWS + 1, 16, 2.0, 1.0, p, None, p, None) == -3
    assert L.arl_uniformity_fwd_bwd_f32(p + 4, 4, 16, 2.0, 1.0, p, None, p, None) == -4
    assert L.arl_alignment_fwd_bwd_f32(p, None, 4, 16, 2.0, 1.0, p, None, None, p, None) == -1
    assert L.arl_alignment_fwd_bwd_f32(p, p, 4, 18, 2.0, 1.0, p, None, None, p, None) == -2
    assert L.arl_alignment_fwd_bwd_f32(p, p, 4, 260, 2.0, 1.0, p, None, None, p, None) == -2
    assert L.arl_alignment_fwd_bwd_f32(p, p, 4, 16, 2.0, 1.0, p, p, None, p, None) == -4
    assert L.arl_alignment_fwd_bwd_f32(p, p, 0, 16, 2.0, 1.0, p, None, None, p, None) == -4
    # the split rule: one split below its row floor, a count that never drops as the table grows, nothing outside the limits
    assert L.arl_uniformity_splits(1) == 0 and L.arl_uniformity_splits(pairloss.PAIRLOSS_MAX_ROWS + 1) == 0 and L.arl_uniformity_splits(2) == 1
    n2 = int(g33()['unif_shapes'][4][0])
    assert L.arl_uniformity_splits(n2 - 1) == 1 and L.arl_uniformity_splits(n2) == 2
    assert L.arl_uniformity_workspace_bytes(1, 16) == 0 and L.arl_uniformity_workspace_bytes(64, 24) == 0
    assert L.arl_uniformity_workspace_bytes(2048, 64) % 16 == 0 and L.arl_uniformity_workspace_bytes(2048, 64) >= 4 * (2 + L.arl_uniformity_splits(2048)) * 2048 * 64


def test_host_and_unsupported_tensors_raise_in_the_op_module():
    from arlib_amd import pairloss
    with pytest.raises(ValueError, match='GPU'):
        pairloss.uniformity(torch.randn(8, 16))
    with pytest.raises(ValueError, match='float32'):
        pairloss.uniformity(torch.randn(8, 16, dtype=torch.float64))
    with pytest.raises(ValueError, match='width'):
        pairloss.uniformity(torch.randn(8, 24))
    with pytest.raises(ValueError, match='GPU'):
        pairloss.alignment(torch.randn(8, 16), torch.randn(8, 16))
    with pytest.raises(ValueError, match='width'):
        pairloss.alignment(torch.randn(8, 18), torch.randn(8, 18))


def test_restated_kernel_formula_equals_reference_float64():
    """dist^2 from q and s, the masked diagonal and -4 t / S: what the GPU test feeds its bounds with is the reference's float64 value."""
    g = g33()
    for name, n, d in unif_sets(g):
        lo, gx = uniformity_restated(unif_input(g, name))
        assert abs(lo - float(g[name + '__loss64'])) <= F64_TOL, name
        assert rel(pick(gx, g, name + '__grad64'), g[name + '__grad64']) <= F64_TOL, name
        if 'clust' in name and n > 3:
            got, ref = pick(gx, g, name + '__grad64'), g[name + '__grad64']
            err = np.linalg.norm(got - ref, axis=1)
            assert np.all(err <= 1e-7 * np.linalg.norm(ref, axis=1)), name          # row by row: the zero row's gradient is 10^12 times the others
    lo, gx = uniformity_restated(unif_input(g, 'unif_clust_2x16'))
    assert not gx.any()                                                             # two identical rows: the gradient is exactly zero

"""The pair-loss kernels (arlib_amd/pairloss.py, csrc/arl_pairloss.hip) on the MI355X against float64: every input set of g33_pairloss.npz through
pairloss.uniformity and pairloss.alignment, held to the reference's own fp32 error (stored in the fixture) times 4 -- the allowance for another
summation order -- or 16 ulp of fp32, whichever is larger; then determinism, the upstream factor, the util.loss Functions and the routes around the
kernel.  The float64 values are those of tests/test_pairloss_cpu.uniformity_restated, which that file pins to the reference's float64 autograd.

Measured on the MI355X (|loss - loss64| and ||dX - g64|| / ||g64||, kernel / reference fp32): DESIGN.md section 3i has the table."""
import numpy as np
import pytest
import torch
from conftest import golden
from test_ncf_wrmf_cpu import pick
from test_pairloss_cpu import unif_sets, unif_input, uniformity_restated

pytestmark = pytest.mark.gpu
DEV = 'cuda'
ULP16 = 16 * 2.0 ** -23
G33 = golden('g33_pairloss.npz')
SETS = unif_sets(G33)
_cache = {}


@pytest.fixture(scope='module', autouse=True)
def need_gpu():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU')


def unif_case(name):
    """(x on the device, loss64, g64) of a set; the float64 side is computed once and shared."""
    if name not in _cache:
        x = unif_input(G33, name)
        l64, g64 = uniformity_restated(x)
        g64.setflags(write=False)
        _cache[name] = (torch.from_numpy(x).to(DEV), l64, g64)
    return _cache[name]


@pytest.mark.parametrize('name,n,d', SETS, ids=[s[0] for s in SETS])
def test_uniformity_against_float64_within_the_reference_error(name, n, d):
    from arlib_amd import pairloss
    x, l64, g64 = unif_case(name)
    loss, dX = pairloss.uniformity(x)
    loss_only, none = pairloss.uniformity(x, want_grad=False)
    assert none is None and torch.equal(loss, loss_only)
    got, dX = float(loss), dX.cpu().numpy().astype(np.float64)
    ref_loss_err, ref_grad_err, ref_row_err = float(G33[name + '__loss_err']), float(G33[name + '__grad_err']), G33[name + '__grad_rowerr']
    err, norm = np.linalg.norm(dX - g64), np.linalg.norm(g64)
    row_err, row_norm = np.linalg.norm(dX - g64, axis=1), np.linalg.norm(g64, axis=1)
    row_rel = np.where(row_norm > 0, row_err / np.where(row_norm > 0, row_norm, 1.0), row_err)
    print('%s: loss err %.2e (reference fp32 %.2e)  gradient err %.2e (reference fp32 %.2e)  worst row %.2e (reference fp32 %.2e)'
          % (name, abs(got - l64), ref_loss_err, err / norm if norm > 0 else err, ref_grad_err, row_rel.max(), ref_row_err.max()))
    assert np.isfinite(dX).all()
    assert abs(got - l64) <= max(4 * ref_loss_err, ULP16 * max(1.0, abs(l64)))
    assert err <= max(4 * ref_grad_err, ULP16) * norm
    if 'clust' in name:
        # row by row, every row against the reference's fp32 error on THAT row: the zero row's gradient is 10^12 times the others and alone decides the norm above
        assert np.all(row_err <= np.maximum(4 * ref_row_err, ULP16) * row_norm), np.flatnonzero(row_err > np.maximum(4 * ref_row_err, ULP16) * row_norm)
        if n > 3:
            assert row_norm[3] > 1e9 * np.median(row_norm)


def test_stored_gradient_rows_are_what_the_restatement_gives():
    for name, n, d in SETS:
        _, l64, g64 = unif_case(name)
        assert abs(l64 - float(G33[name + '__loss64'])) <= 1e-9
        assert np.linalg.norm(pick(g64, G33, name + '__grad64') - G33[name + '__grad64']) <= 1e-9 * max(np.linalg.norm(G33[name + '__grad64']), 1e-300)


def test_two_runs_are_bit_identical_and_the_input_is_untouched():
    from arlib_amd import pairloss
    for name in ('unif_gauss_1061x128', 'unif_clust_%dx%d' % SETS[4][1:]):
        x = unif_case(name)[0]
        keep = x.clone()
        a, b = pairloss.uniformity(x), pairloss.uniformity(x)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(x, keep)
    xa, ya = (torch.from_numpy(G33['align_130x64__' + k]).to(DEV) for k in 'xy')
    a, b = pairloss.alignment(xa, ya), pairloss.alignment(xa, ya)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_upstream_scales_the_gradient_exactly():
    from arlib_amd import pairloss
    x = unif_case('unif_gauss_130x64')[0]
    loss1, g1 = pairloss.uniformity(x)
    for up in (0.25, -8.0):                                               # powers of two: the product is exact wherever it is applied
        loss, g = pairloss.uniformity(x, upstream=up)
        assert torch.equal(loss, loss1) and torch.equal(g, g1 * up)
    _, g = pairloss.uniformity(x, upstream=3.0)                           # any other factor: one rounding of the product, applied before the division by the norm
    assert torch.allclose(g, g1 * 3.0, rtol=4 * 2.0 ** -23, atol=0)
    _, g0 = pairloss.uniformity(x, upstream=0.0)
    assert not g0.any()


def composed(fn, dtype, *arrays):
    """The composed (reference) expression on the CPU in `dtype`: (loss, gradients as float64 numpy)."""
    ts = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in arrays]
    loss = fn(*ts)
    return loss.item(), [g.double().numpy() for g in torch.autograd.grad(loss, ts)]


def bounds(fn, *arrays):
    """(loss64, grads64, loss bound, gradient bounds) with the rule of this file: 4 times the composed fp32 route's own error, or 16 ulp."""
    l32, g32 = composed(fn, torch.float32, *arrays)
    l64, g64 = composed(fn, torch.float64, *arrays)
    gb = [max(4 * np.linalg.norm(a - b) / np.linalg.norm(b), ULP16) for a, b in zip(g32, g64)]
    return l64, g64, max(4 * abs(l32 - l64), ULP16 * max(1.0, abs(l64))), gb


def test_other_temperatures_against_float64():
    from arlib_amd import pairloss
    x = unif_case('unif_gauss_17x16')[0]
    for t in (0.5, 3):
        fn = lambda z: torch.pdist(torch.nn.functional.normalize(z, dim=-1), p=2).pow(2).mul(-t).exp().mean().log()
        l64, (g64,), lb, (gb,) = bounds(fn, x.cpu().numpy())
        r64 = uniformity_restated(x.cpu().numpy(), t=float(t))
        assert abs(r64[0] - l64) <= 1e-9 and np.linalg.norm(r64[1] - g64) <= 1e-9 * np.linalg.norm(g64)
        loss, dX = pairloss.uniformity(x, t=t)
        assert abs(float(loss) - l64) <= lb
        assert np.linalg.norm(dX.cpu().numpy() - g64) <= gb * np.linalg.norm(g64)


@pytest.mark.parametrize('alpha', [1, 2])
def test_alignment_against_float64_and_the_identical_pair(alpha):
    from arlib_amd import pairloss
    k = 'align_130x64_a%d__' % alpha
    x, y = (torch.from_numpy(G33['align_130x64__' + s]).to(DEV) for s in 'xy')
    loss, dX, dY = pairloss.alignment(x, y, alpha)
    l64 = float(G33[k + 'loss64'])
    err = abs(float(loss) - l64)
    ex = np.linalg.norm(pick(dX, G33, k + 'gradx64') - G33[k + 'gradx64']) / np.linalg.norm(G33[k + 'gradx64'])
    ey = np.linalg.norm(pick(dY, G33, k + 'grady64') - G33[k + 'grady64']) / np.linalg.norm(G33[k + 'grady64'])
    print('alignment alpha %d: loss err %.2e (reference fp32 %.2e)  gradient err %.2e / %.2e (reference fp32 %.2e / %.2e)'
          % (alpha, err, float(G33[k + 'loss_err']), ex, ey, float(G33[k + 'gradx_err']), float(G33[k + 'grady_err'])))
    assert err <= max(4 * float(G33[k + 'loss_err']), ULP16 * max(1.0, abs(l64)))
    assert ex <= max(4 * float(G33[k + 'gradx_err']), ULP16) and ey <= max(4 * float(G33[k + 'grady_err']), ULP16)
    r = int(G33['align_130x64__same_row'])
    assert not dX[r].any() and not dY[r].any() and torch.isfinite(dX).all() and torch.isfinite(dY).all()      # 0, not NaN, at the origin of the norm
    loss_only, n1, n2 = pairloss.alignment(x, y, alpha, want_grad=False)
    assert n1 is None and n2 is None and torch.equal(loss_only, loss)


def test_alignment_widths_zero_rows_and_many_rows():
    """One lane group, a ragged last float4 lane, the widest row, and more rows than one sweep of the grid (4 x 65 536)."""
    from arlib_amd import pairloss
    g = torch.Generator().manual_seed(5)
    fn = lambda a, b: (torch.nn.functional.normalize(a, dim=-1) - torch.nn.functional.normalize(b, dim=-1)).norm(p=2, dim=1).pow(2).mean()
    for n, d in ((1, 4), (7, 36), (1030, 256), (262200, 4)):
        x, y = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
        if n > 2:
            x[2] = 0.0                                                    # a zero row stays zero under the normalisation; its gradient is 10^12 times the others
        l64, (gx, gy), lb, (bx, by) = bounds(fn, x.numpy(), y.numpy())
        loss, dX, dY = pairloss.alignment(x.to(DEV), y.to(DEV))
        dX, dY = dX.cpu().double().numpy(), dY.cpu().double().numpy()
        assert abs(float(loss) - l64) <= lb
        assert np.linalg.norm(dX - gx) <= bx * np.linalg.norm(gx) and np.linalg.norm(dY - gy) <= by * np.linalg.norm(gy)
        if n > 2:                                                         # without the zero row, which alone decides the norm above
            keep = np.arange(n) != 2
            l32, (hx, _) = composed(fn, torch.float32, x.numpy(), y.numpy())
            rest = max(4 * np.linalg.norm(hx[keep] - gx[keep]) / np.linalg.norm(gx[keep]), ULP16)
            assert np.linalg.norm(dX[keep] - gx[keep]) <= rest * np.linalg.norm(gx[keep])


def test_functions_under_autograd_equal_the_op():
    from arlib_amd import pairloss
    from arlib_amd.util import loss as L
    x = unif_case('unif_gauss_130x64')[0]
    xr = x.clone().requires_grad_(True)
    lo = L.uniformity_loss(xr)
    (gx,) = torch.autograd.grad(lo * 0.5, xr)
    loss, dX = pairloss.uniformity(x)
    assert lo.dim() == 0 and torch.equal(lo.detach(), loss[0]) and torch.equal(gx, dX * 0.5)
    xa, ya = (torch.from_numpy(G33['align_130x64__' + k]).to(DEV).requires_grad_(True) for k in 'xy')
    la = L.alignment_loss(xa, ya, alpha=1)
    ga = torch.autograd.grad(la, (xa, ya))
    loss, dX, dY = pairloss.alignment(xa.detach(), ya.detach(), 1)
    assert torch.equal(la.detach(), loss[0]) and torch.equal(ga[0], dX) and torch.equal(ga[1], dY)
    # non-contiguous rows (what indexing a table gives is contiguous; a column slice is not) reach the kernel as contiguous copies
    wide = torch.randn(40, 64, device=DEV)
    assert torch.equal(L.uniformity_loss(wide[:, :32]), L.uniformity_loss(wide[:, :32].contiguous()))
    # batch_softmax_loss is InfoNCE's arithmetic on InfoNCE's kernel
    a, b = (torch.from_numpy(G33['bsm__' + k]).to(DEV).requires_grad_(True) for k in 'ab')
    lb = L.batch_softmax_loss(a, b, 0.2)
    gb = torch.autograd.grad(lb, (a, b))
    assert torch.equal(lb, L.InfoNCE(a, b, 0.2)) and abs(lb.item() - float(G33['bsm__loss64'])) <= 1e-5 * abs(float(G33['bsm__loss64']))
    for got, key in zip(gb, ('bsm__grada64', 'bsm__gradb64')):
        assert np.linalg.norm(got.cpu().numpy() - G33[key]) <= 1e-4 * np.linalg.norm(G33[key])
    for fn, key in ((L.kl_divergence, 'kl'), (L.js_divergence, 'js')):
        assert abs(fn(a.detach(), b.detach()).item() - float(G33[key + '__loss64'])) <= 1e-5 * abs(float(G33[key + '__loss64']))


def test_routes_around_the_kernel_and_errors(monkeypatch):
    from arlib_amd import pairloss
    from arlib_amd.util import loss as L
    calls = {'u': 0, 'a': 0}
    real_u, real_a = pairloss.uniformity, pairloss.alignment
    monkeypatch.setattr(pairloss, 'uniformity', lambda *a, **k: (calls.__setitem__('u', calls['u'] + 1), real_u(*a, **k))[1])
    monkeypatch.setattr(pairloss, 'alignment', lambda *a, **k: (calls.__setitem__('a', calls['a'] + 1), real_a(*a, **k))[1])
    g = torch.Generator().manual_seed(9)
    x24, y24 = torch.randn(50, 24, generator=g).to(DEV), torch.randn(50, 24, generator=g).to(DEV)
    ref = torch.pdist(torch.nn.functional.normalize(x24.double(), dim=-1)).pow(2).mul(-2).exp().mean().log().item()
    assert abs(L.uniformity_loss(x24).item() - ref) <= 1e-5 and calls['u'] == 0                  # width outside the list: composed
    L.alignment_loss(x24, y24)
    assert calls['a'] == 1                                                                      # ... which alignment's kernel covers
    x18 = torch.randn(50, 18, generator=g).to(DEV)
    L.alignment_loss(x18, x18 * 0.5 + 1.0)
    assert calls['a'] == 1                                                                      # not a multiple of 4: composed
    assert torch.isnan(L.uniformity_loss(x24[:1, :16].contiguous())) and calls['u'] == 0        # one row: the reference's NaN
    L.uniformity_loss(x24.cpu()[:, :16].contiguous()); L.uniformity_loss(x24[:, :16].double())
    assert calls['u'] == 0                                                                      # host and float64 tensors: composed
    L.uniformity_loss(x24[:, :16].contiguous())
    assert calls['u'] == 1
    with pytest.raises(ValueError, match='width'):
        real_u(x24)
    with pytest.raises(ValueError, match='rows'):
        real_u(x24[:1, :16].contiguous())
    with pytest.raises(ValueError, match='GPU'):
        real_u(x24.cpu()[:, :16].contiguous())
    with pytest.raises(ValueError, match='float32'):
        real_a(x24.double(), y24.double())
    with pytest.raises(ValueError, match='one device'):
        real_a(x24, y24[:10])


def test_no_gradient_wanted_means_the_forward_launch_alone(monkeypatch):
    """Under no_grad or on detached rows the util.loss functions ask the op for the loss only: a table-scale diagnostic pays neither the second
    product nor its workspace, and gets the bits of the differentiable call."""
    from arlib_amd import pairloss
    from arlib_amd.util import loss as L
    asked = []
    real_u, real_a = pairloss.uniformity, pairloss.alignment
    monkeypatch.setattr(pairloss, 'uniformity', lambda x, t=2, want_grad=True, upstream=None: (asked.append(want_grad), real_u(x, t, want_grad, upstream))[1])
    monkeypatch.setattr(pairloss, 'alignment', lambda x, y, alpha=2, want_grad=True: (asked.append(want_grad), real_a(x, y, alpha, want_grad))[1])
    x = unif_case('unif_gauss_130x64')[0]
    xr, yr = x.clone().requires_grad_(True), (x.flip(0) * 0.5 + 0.25).requires_grad_(True)
    with torch.no_grad():
        lu, la = L.uniformity_loss(xr), L.alignment_loss(xr, yr)
    assert asked == [False, False] and not lu.requires_grad and not la.requires_grad
    assert torch.equal(L.uniformity_loss(x), lu) and torch.equal(L.alignment_loss(xr.detach(), yr.detach()), la) and asked == [False] * 4
    lu2, la2 = L.uniformity_loss(xr), L.alignment_loss(xr.detach(), yr)
    assert asked[4:] == [True, True] and torch.equal(lu2.detach(), lu) and torch.equal(la2.detach(), la)
    gx, gy = torch.autograd.grad(lu2 + la2, (xr, yr))
    assert torch.equal(gx, real_u(x)[1]) and torch.equal(gy, real_a(x, yr.detach())[2])

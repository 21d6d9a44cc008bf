"""DirectAU's two loss terms on the device (csrc/arl_pairloss.hip; reference util/loss.py:17-23, alignment_loss / uniformity_loss) as tensor-level
ops, forward and backward in one call each.  Inputs are RAW rows: the kernels normalise them.  A module of its own like arlib_amd/cluster.py and
arlib_amd/colsoftmax.py, with its poisoned-memory sweep in tests/test_gpu_pairloss_poison.py.  DESIGN.md section 3i has the rules."""
import torch

from . import _lib, ops
from ._lib import check

PAIRLOSS_WIDTHS = ops.NCE_ALLROWS_WIDTHS          # uniformity: the widths of the exact-fp32 MFMA tile kernels
PAIRLOSS_MAX_ROWS = (2 ** 31 - 1) // 128         # every row * d offset of the kernels' index arithmetic stays in int32
ALIGNMENT_MAX_WIDTH = 256                        # alignment: one wave holds a row as float4s


def _rows(t, name, what, min_rows, widths=None):
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError('%s: %s must be a 2-d torch.Tensor' % (what, name))
    d = t.shape[1]
    if (d not in widths) if widths is not None else (d < 4 or d % 4 or d > ALIGNMENT_MAX_WIDTH):
        raise ValueError('%s: width %d outside %s' % (what, d, widths if widths is not None else 'the multiples of 4 up to %d' % ALIGNMENT_MAX_WIDTH))
    if t.dtype != torch.float32:
        raise ValueError('%s: %s must be float32, got %s' % (what, name, t.dtype))
    if not t.is_cuda:
        raise ValueError('%s: %s must be on the GPU (there is no host route), got %s' % (what, name, t.device))
    if not min_rows <= t.shape[0] <= PAIRLOSS_MAX_ROWS:
        raise ValueError('%s: %s needs %d <= rows <= %d' % (what, name, min_rows, PAIRLOSS_MAX_ROWS))
    return t.contiguous()


def uniformity_splits(n):
    """Splits of the streamed side at n rows (their partial sums are added in split order); 0 outside 2 <= n <= PAIRLOSS_MAX_ROWS."""
    return int(_lib.lib().arl_uniformity_splits(int(n)))


def uniformity(x, t=2, want_grad=True, upstream=None):
    """(loss [1], dX | None) for loss = log(mean_{i<j} exp(-t |y_i - y_j|^2)), y = F.normalize(x) -- util/loss.py:21-23 and its autograd on raw rows
    x [n, d] (float32, on the GPU, d in PAIRLOSS_WIDTHS, 2 <= n <= PAIRLOSS_MAX_ROWS) without the n (n - 1) / 2 distances of torch.pdist.
    dX = upstream * dloss/dx (upstream: a number, None = 1).  Bit-identical from run to run.  ValueError for anything else: there is no other route."""
    x = _rows(x, 'x', 'uniformity', 2, PAIRLOSS_WIDTHS)
    if not float(t) > 0:
        raise ValueError('uniformity: t = %r, a positive number needed' % (t,))
    n, d = x.shape
    L = _lib.lib()
    ws = torch.empty(L.arl_uniformity_workspace_bytes(n, d), dtype=torch.uint8, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dX = torch.empty_like(x) if want_grad else None
    check(L.arl_uniformity_fwd_bwd_f32(ops._ptr(x), n, d, float(t), 1.0 if upstream is None else float(upstream), ops._ptr(loss), ops._ptr(dX), ops._ptr(ws),
                                       ops._stream()), 'arl_uniformity_fwd_bwd_f32')
    return loss, dX


def alignment(x, y, alpha=2, want_grad=True):
    """(loss [1], dX, dY) for loss = mean_b |x^_b - y^_b|^alpha, x^ = F.normalize(x) -- util/loss.py:17-19 and its autograd on raw rows x, y [n, d]
    (float32, on the GPU, d a multiple of 4 up to 256, n >= 1).  A pair with x^_b == y^_b has zero gradient rows.  dX = dY = None without want_grad."""
    x, y = _rows(x, 'x', 'alignment', 1), _rows(y, 'y', 'alignment', 1)
    if x.shape != y.shape or x.device != y.device:
        raise ValueError('alignment: x and y [n, d] on one device')
    if not float(alpha) > 0:
        raise ValueError('alignment: alpha = %r, a positive number needed' % (alpha,))
    n, d = x.shape
    terms = torch.empty(n, dtype=torch.float32, device=x.device)
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    dX, dY = (torch.empty_like(x), torch.empty_like(y)) if want_grad else (None, None)
    check(_lib.lib().arl_alignment_fwd_bwd_f32(ops._ptr(x), ops._ptr(y), n, d, float(alpha), 1.0, ops._ptr(loss), ops._ptr(dX), ops._ptr(dY), ops._ptr(terms),
                                               ops._stream()), 'arl_alignment_fwd_bwd_f32')
    return loss, dX, dY

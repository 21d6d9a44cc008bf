"""APR's adversarial BPR term (csrc/arl_advpair.hip): the tensor-level wrapper over arl_bpr_adv_fwd_bwd_f32, also reachable as
ops.bpr_adv_fwd_bwd / ops.bpr_adv_supported.  Argument checks follow ops.bpr_l2_fwd_bwd."""
import torch

from . import _lib
from ._lib import check
from .ops import _dev, _ptr, _stream, _check_idx

BPR_ADV_MAX_BATCH = 16384 // 3       # arl_bpr_adv_fwd_bwd_f32's limit: the 3B positions are one window of the ownership scan
BPR_ADV_MAX_WIDTH = 256


def bpr_adv_supported(B, d):
    """Shapes arl_bpr_adv_fwd_bwd_f32 takes: 1 <= B <= 5461 samples, 1 <= d <= 256."""
    return 1 <= B <= BPR_ADV_MAX_BATCH and 1 <= d <= BPR_ADV_MAX_WIDTH


def bpr_adv_fwd_bwd(emb, item_off, u, p, n, eps, groups=None, G=None, upstream=1.0, delta_out=None, workspace=None, loss_out=None, check_range=True,
                    distinct_rows=False):
    """APR's adversarial BPR term on rows gathered from the combined table (include/arlib_amd.h); returns loss_out = [adv, clean bpr] (device).
    groups: int32 [3B] node of each position (users, positives, negatives), None: the gathered row id, or the position with distinct_rows.
    If G is given, upstream * d adv / d emb (the perturbation held constant) is added into it, duplicates in position order (no float atomics).
    delta_out: optional [3B, d], receives each position's perturbation.  distinct_rows as in bpr_l2_fwd_bwd."""
    _dev(emb, torch.float32, 'emb', 2)
    N, d = emb.shape
    B = u.numel()
    for t, nm in ((u, 'u'), (p, 'p'), (n, 'n')):
        _check_idx(t, nm, N, B)
        if t.device != emb.device:
            raise ValueError('bpr_adv: %s on %s, emb on %s' % (nm, t.device, emb.device))
    if B == 0:
        raise ValueError('bpr_adv: empty batch')
    if not bpr_adv_supported(B, d):
        raise ValueError('bpr_adv: B = %d, d = %d unsupported (B <= %d, d <= %d)' % (B, d, BPR_ADV_MAX_BATCH, BPR_ADV_MAX_WIDTH))
    if not float(eps) >= 0.0:
        raise ValueError('bpr_adv: eps >= 0')
    if groups is not None:
        _check_idx(groups, 'groups', None, 3 * B)
        if groups.device != emb.device:
            raise ValueError('bpr_adv: groups on %s, emb on %s' % (groups.device, emb.device))
    if check_range:   # host-side bounds check (one small sync); hot loops validate once and pass check_range=False
        mx = torch.stack([u.max(), p.max(), n.max(), -u.min(), -p.min(), -n.min()]).tolist()
        if mx[0] >= N or max(mx[1], mx[2]) + item_off >= N or max(mx[3:]) > 0:
            raise IndexError('bpr_adv: batch index out of range')
        if groups is not None and int(groups.min()) < 0:
            raise IndexError('bpr_adv: group id out of range (ids are >= 0)')
    for t, nm, shape in ((G, 'G', tuple(emb.shape)), (delta_out, 'delta_out', (3 * B, d))):
        if t is not None:
            _dev(t, torch.float32, nm, 2)
            if tuple(t.shape) != shape or t.device != emb.device:
                raise ValueError('bpr_adv: %s must be %s on the device of emb' % (nm, shape))
    need = _lib.lib().arl_bpr_adv_workspace_bytes(B, d)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = torch.empty(need // 4, dtype=torch.float32, device=emb.device)
    if loss_out is None:
        loss_out = torch.empty(2, dtype=torch.float32, device=emb.device)
    check(_lib.lib().arl_bpr_adv_fwd_bwd_f32(_ptr(emb), d, item_off, _ptr(u), _ptr(p), _ptr(n), B, _ptr(groups), float(eps), float(upstream), _ptr(loss_out),
                                             _ptr(G), _ptr(delta_out), _ptr(workspace), 1 if distinct_rows else 0, _stream()), 'arl_bpr_adv_fwd_bwd_f32')
    return loss_out

"""GOAT's co-rating degree (csrc/arl_corating.hip; reference attack/Gray/GOAT.py:37-39) as a tensor-level op: itemIntNum[j] = the number of items
that share at least one user with item j, without the I x I product the reference forms.  A module of its own like arlib_amd/cluster.py, with its
poisoned-memory sweep in tests/test_gpu_goat_poison.py.  DESIGN.md section 3h has the rules."""
import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from ._lib import check

CORATING_MAX_ITEMS = (160 * 1024 // 4 - 16) * 32          # bits of the LDS bitmap: 160 KiB minus the kernel's 16 words (arl_corating_max_items)


def _ops():
    from . import ops
    return ops


def corating_degree_supported(n_items):
    """True when the bitmap of n_items bits fits the LDS of one workgroup; past it corating_degree_host is the route."""
    return 0 <= int(n_items) <= CORATING_MAX_ITEMS


def _item_major(rp, ci, n_users, n_items):
    """(i_colptr int64 [I + 1], i_row int32 [nnz], order int32 [I]) of the CSR (rp, ci) on its device: the item-major index (users ascending within an
    item) and the launch order, items by the summed degrees of their users -- the ORs the item's workgroup issues -- heaviest first."""
    dev, cl, deg = rp.device, ci.long(), rp[1:] - rp[:-1]
    rows = torch.repeat_interleave(torch.arange(n_users, device=dev), deg)
    i_row = rows[torch.sort(cl, stable=True).indices].to(torch.int32).contiguous()
    i_colptr = torch.zeros(n_items + 1, dtype=torch.int64, device=dev)
    i_colptr[1:] = torch.cumsum(torch.bincount(cl, minlength=n_items), 0)
    weight = torch.zeros(n_items, dtype=torch.int64, device=dev).index_add_(0, cl, deg[rows])
    return i_colptr, i_row, torch.sort(weight, descending=True, stable=True).indices.to(torch.int32).contiguous()


def corating_degree(rowptr, col, n_users, n_items, device='cuda'):
    """int32 [n_items] on the device: out[j] = the number of distinct items i (j included) with a common user with item j, 0 for an item nobody
    rated -- ((X.T @ X) > 0).sum(0) of the n_users x n_items matrix X given as CSR (rowptr [n_users + 1], col [nnz]; tensors or arrays, any
    order within a row, repeated entries allowed).  The item-major index and the launch order (heaviest item first, by the summed degrees of its
    users) are built here.  ValueError past corating_degree_supported or for ids out of range: the kernel trusts what it is given."""
    o = _ops()
    n_users, n_items = int(n_users), int(n_items)
    if n_users < 0 or n_items < 0 or n_users >= 2 ** 31:
        raise ValueError('corating_degree: n_users = %d, n_items = %d' % (n_users, n_items))
    if not corating_degree_supported(n_items):
        raise ValueError('corating_degree: %d items, the LDS bitmap holds %d: use corating_degree_host' % (n_items, CORATING_MAX_ITEMS))
    dev = rowptr.device if isinstance(rowptr, torch.Tensor) and rowptr.is_cuda else torch.device(device)
    rp = torch.as_tensor(rowptr).to(dev, torch.int64).contiguous()
    ci = torch.as_tensor(col).to(dev, torch.int32).contiguous()
    nnz = ci.numel()
    if rp.dim() != 1 or ci.dim() != 1 or rp.numel() != n_users + 1 or nnz >= 2 ** 31:
        raise ValueError('corating_degree: rowptr [n_users + 1] and col [nnz < 2^31] needed')
    deg = rp[1:] - rp[:-1]
    if int(rp[0]) != 0 or int(rp[-1]) != nnz or (n_users and int(deg.min()) < 0):
        raise ValueError('corating_degree: rowptr must rise from 0 to nnz')
    if nnz and (int(ci.min()) < 0 or int(ci.max()) >= n_items):
        raise ValueError('corating_degree: item id outside [0, %d)' % n_items)
    out = torch.empty(n_items, dtype=torch.int32, device=dev)
    if n_items == 0:
        return out
    i_colptr, i_row, order = _item_major(rp, ci, n_users, n_items)
    check(_lib.lib().arl_corating_degree_i32(o._ptr(rp), o._ptr(ci), o._ptr(i_colptr), o._ptr(i_row), n_users, n_items, o._ptr(order), o._ptr(out),
                                             o._stream()), 'arl_corating_degree_i32')
    return out


def corating_degree_host(interact):
    """The reference's expression (GOAT.py:37-39) on the host, as a float64 array [I]: the item-item product, every stored entry set to 1, column
    sums.  For catalogues past corating_degree_supported and as the yardstick of the tests; scipy holds the I x I product, so it ends where
    that no longer fits."""
    X = sp.csr_matrix(interact)
    M = (X.T @ X).tocsr()
    M.data = (M.data > 0).astype(np.float64)
    return np.asarray(M.sum(0), dtype=np.float64).ravel()

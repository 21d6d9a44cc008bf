"""AUSH's GAN steps (reference attack/Gray/AUSH.py:55-115) on the arl_gan_* kernels, and the same steps composed from torch ops (the route
past the kernels' limits, ops.gan_supported, and the yardstick of the tests and tools/aush_bench.py).

Shapes: template T [F, S] (sparse; S = I // 5 + T selected items, the targets last), G = Linear(S, S) -> ReLU -> Linear(S, S) -> Sigmoid,
D = Linear(S, 1) -> Sigmoid.
  D step: loss1 = -(mean log D(T) + mean log(1 - D(G(T)))), D stepped.  The reference's backward also reaches G, but optimize_G.zero_grad()
          precedes every G backward, so those gradients are never used: both routes skip them.
  G step: loss2 = mean log D(T) + mean log(1 - D(Y)) + mean_r (sum_{t in targets} (1 - Y[r, t]))^2 + mean (Y - T)^2, Y = G(T), G stepped.
"""
import torch
import torch.nn.functional as Fn

from ... import ops


class Template:
    """One step's template on the device: CSR (rowptr, col, val) in the interaction rows' order, its dense image Td [F, S] and its column-major
    index (CSC: rows = template columns) for dW1."""

    def __init__(self, rowptr, col, val, S):
        self.rowptr, self.col, self.val, self.F, self.S = rowptr, col, val, rowptr.numel() - 1, int(S)
        r = torch.repeat_interleave(torch.arange(self.F, device=rowptr.device), rowptr[1:] - rowptr[:-1])
        self.row = r
        self.Td = torch.zeros(self.F, self.S, dtype=torch.float32, device=rowptr.device)
        self.Td[r, col.long()] = val                                          # (row, col) pairs are unique
        order = torch.sort(col.long() * self.F + r).indices                   # column-major, rows ascending within a column
        self.csc_ptr = torch.zeros(self.S + 1, dtype=torch.int64, device=rowptr.device)
        torch.cumsum(torch.bincount(col.long(), minlength=self.S), 0, out=self.csc_ptr[1:])
        self.csc_row = r[order].to(torch.int32).contiguous()
        self.csc_val = val[order].contiguous()

    def sparse(self):
        return torch.sparse_coo_tensor(torch.stack([self.row, self.col.long()]), self.val, (self.F, self.S)).coalesce()


def _params(G, D):
    l0, l1, d0 = G.net.layer_0, G.net.layer_1, D.net[0]
    return l0.weight, l0.bias, l1.weight, l1.bias, d0.weight, d0.bias


def fused_forward(G, D, tpl, n_targets):
    """H = relu(T W1^T + b1), Y = sigmoid(H W2^T + b2) and the per-row partials / losses (ops.gan_rows)."""
    W1, b1, W2, b2, wD, bD = _params(G, D)
    W1t = ops.gan_transpose(W1.detach())
    H = ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, W1t, bias=b1.detach(), relu=True, check_range=False)
    Y = ops.gan_gemm(H, W2.detach(), trans_b=True, epilogue=ops.GAN_EPI_BIAS_SIGMOID, bias=b2.detach())
    rows, losses, coef, pf = ops.gan_rows(Y, tpl.Td, n_targets, wD.detach(), bD.detach())
    return H, Y, rows, losses, coef, pf


def fused_d_grads(G, D, tpl, n_targets):
    """(loss1, dwD, dbD) of one D step."""
    H, Y, rows, losses, coef, pf = fused_forward(G, D, tpl, n_targets)
    F = tpl.F
    dwD = ops.gan_colsum(tpl.Td, coef[:F], Y, coef[F:]).view(1, -1)
    return losses[0:1], dwD, losses[2:3].clone()


def fused_g_grads(G, D, tpl, n_targets):
    """(loss2, dW1, db1, dW2, db2) of one G step."""
    W1, b1, W2, b2, wD, bD = _params(G, D)
    H, Y, rows, losses, coef, pf = fused_forward(G, D, tpl, n_targets)
    dZ2 = ops.gan_dz2(Y, tpl.Td, rows, pf, wD.detach(), n_targets)
    dW2 = ops.gan_gemm(dZ2, H, trans_a=True)
    db2 = ops.gan_colsum(dZ2)
    dZ1 = ops.gan_gemm(dZ2, W2.detach(), epilogue=ops.GAN_EPI_RELU_MASK, aux=H)
    db1 = ops.gan_colsum(dZ1)
    dW1t = ops.gan_spmm(tpl.csc_ptr, tpl.csc_row, tpl.csc_val, dZ1, check_range=False)
    return losses[1:2], ops.gan_transpose(dW1t), db1, dW2, db2


def composed_d_grads(G, D, tpl, n_targets):
    W1, b1, W2, b2, wD, bD = _params(G, D)
    with torch.no_grad():
        Y = torch.sigmoid(Fn.linear(torch.relu(torch.sparse.mm(tpl.sparse(), W1.detach().t()) + b1), W2, b2))
    w, b = wD.detach().requires_grad_(True), bD.detach().requires_grad_(True)
    loss = -(torch.log(torch.sigmoid(Fn.linear(tpl.Td, w, b))).mean() + torch.log(1 - torch.sigmoid(Fn.linear(Y, w, b))).mean())
    gw, gb = torch.autograd.grad(loss, (w, b))
    return loss.detach().view(1), gw, gb


def composed_g_grads(G, D, tpl, n_targets):
    W1, b1, W2, b2, wD, bD = _params(G, D)
    ps = [p.detach().requires_grad_(True) for p in (W1, b1, W2, b2)]
    Y = torch.sigmoid(Fn.linear(torch.relu(torch.sparse.mm(tpl.sparse(), ps[0].t()) + ps[1]), ps[2], ps[3]))
    dD = lambda x: torch.sigmoid(Fn.linear(x, wD.detach(), bD.detach()))
    shill = (1 - Y[:, tpl.S - n_targets:]).sum(1)
    loss = torch.log(dD(tpl.Td)).mean() + torch.log(1 - dD(Y)).mean() + (shill ** 2).mean() + ((Y - tpl.Td) ** 2).mean()
    grads = torch.autograd.grad(loss, ps)
    return (loss.detach().view(1),) + tuple(grads)


def d_step(G, D, opt_D, tpl, n_targets, fused):
    loss, gw, gb = (fused_d_grads if fused else composed_d_grads)(G, D, tpl, n_targets)
    wD, bD = D.net[0].weight, D.net[0].bias
    wD.grad, bD.grad = gw.reshape(wD.shape).contiguous(), gb.reshape(bD.shape).contiguous()
    opt_D.step()
    return loss


def g_step(G, D, opt_G, tpl, n_targets, fused):
    out = (fused_g_grads if fused else composed_g_grads)(G, D, tpl, n_targets)
    for p, g in zip((G.net.layer_0.weight, G.net.layer_0.bias, G.net.layer_1.weight, G.net.layer_1.bias), out[1:]):
        p.grad = g.reshape(p.shape).contiguous()
    opt_G.step()
    return out[0]


@torch.no_grad()
def generate(G, tpl, fused, thr=0.1):
    """Y = G(T) and the CSR (rowptr, col) of Y > thr (the reference's `project`, AUSH.py:144-149)."""
    W1, b1, W2, b2 = G.net.layer_0.weight, G.net.layer_0.bias, G.net.layer_1.weight, G.net.layer_1.bias
    if fused:
        H = ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, ops.gan_transpose(W1), bias=b1, relu=True, check_range=False)
        Y = ops.gan_gemm(H, W2, trans_b=True, epilogue=ops.GAN_EPI_BIAS_SIGMOID, bias=b2)
        rowptr, col = ops.gan_threshold(Y, thr)
        return Y, rowptr, col
    Y = torch.sigmoid(Fn.linear(torch.relu(torch.sparse.mm(tpl.sparse(), W1.t()) + b1), W2, b2))
    r, c = torch.nonzero(Y > thr, as_tuple=True)
    rowptr = torch.zeros(Y.shape[0] + 1, dtype=torch.int64, device=Y.device)
    torch.cumsum(torch.bincount(r, minlength=Y.shape[0]), 0, out=rowptr[1:])
    return Y, rowptr, c.to(torch.int32)

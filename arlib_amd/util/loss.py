"""Loss functions with the reference's names and semantics (util/loss.py: all ten), computed by the HIP
kernels and differentiable through torch.autograd (custom Functions; backward is another kernel, not autograd of
ATen ops).  Inputs are GPU fp32 tensors; there is no CPU fallback (wrmf_loss, alignment_loss and uniformity_loss also take other tensors, as the
reference functions; kl_divergence and js_divergence are on no model's path and are composed from torch ops).  adv_bpr_loss, APR's adversarial term,
is an addition to the reference's ten and also takes other tensors; so is multinomial_nll, the autoencoders' likelihood
(arlib_amd/multinomial.py), whose composed route runs on the CPU too.
"""
import torch
import torch.nn.functional as F

from .. import ops, pairloss
from ..multinomial import multinomial_nll  # noqa: F401


def _i32(t):
    return t if t.dtype == torch.int32 else t.to(torch.int32)


class _BprL2Rows(torch.autograd.Function):
    """bpr_loss(u,p,n) and/or reg*(||u||_F+||p||_F) on already-gathered [B,d] rows (fused kernel over a packed copy)."""

    @staticmethod
    def forward(ctx, user_emb, pos_emb, neg_emb, reg, which):
        B, d = user_emb.shape
        packed = torch.cat([user_emb, pos_emb, neg_emb], 0).contiguous()
        ar = torch.arange(B, dtype=torch.int32, device=packed.device)
        out = ops.bpr_l2_fwd_bwd(packed, B, ar, ar, ar + B, reg, None, check_range=False)
        ctx.save_for_backward(packed)
        ctx.reg, ctx.which, ctx.B = reg, which, B
        return out[0].clone() if which == 'bpr' else (out[1].clone() if which == 'reg' else out[0] + out[1])

    @staticmethod
    def backward(ctx, gout):
        (packed,) = ctx.saved_tensors
        B = ctx.B
        ar = torch.arange(B, dtype=torch.int32, device=packed.device)
        G = torch.zeros_like(packed)
        # the fused kernel produces d(bpr + reg-term); isolate one of them by a second call with reg = 0 when needed
        if ctx.which == 'both':
            ops.bpr_l2_fwd_bwd(packed, B, ar, ar, ar + B, ctx.reg, G, upstream=1.0, check_range=False, distinct_rows=True)
        elif ctx.which == 'bpr':
            ops.bpr_l2_fwd_bwd(packed, B, ar, ar, ar + B, 0.0, G, upstream=1.0, check_range=False, distinct_rows=True)
        else:
            ops.bpr_l2_fwd_bwd(packed, B, ar, ar, ar + B, ctx.reg, G, upstream=1.0, check_range=False, distinct_rows=True)
            G2 = torch.zeros_like(packed)
            ops.bpr_l2_fwd_bwd(packed, B, ar, ar, ar + B, 0.0, G2, upstream=1.0, check_range=False, distinct_rows=True)
            G -= G2
        G *= gout
        return G[:B], G[B:2 * B], G[2 * B:], None, None


def bpr_loss(user_emb, pos_item_emb, neg_item_emb):
    """util/loss.py:5-9: mean(-log(10e-8 + sigmoid(<u,p> - <u,n>)))"""
    return _BprL2Rows.apply(user_emb, pos_item_emb, neg_item_emb, 0.0, 'bpr')


class _FrobNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, emb):
        x = emb.contiguous()
        B = x.shape[0]
        ar = torch.arange(B, dtype=torch.int32, device=x.device)
        out = ops.bpr_l2_fwd_bwd(x, 0, ar, ar, ar, 1.0, None, check_range=False)     # out[2] = ||x||_F
        ctx.save_for_backward(x, out)
        return out[2].clone()

    @staticmethod
    def backward(ctx, gout):
        x, out = ctx.saved_tensors
        # torch.norm's backward gives 0 (not NaN) at the origin; bpr_bwd_kernel guards the same way
        return x * torch.where(out[2] > 0, gout / out[2], torch.zeros_like(gout))


def l2_reg_loss(reg, *args):
    """util/loss.py:25-29: reg * sum_k ||emb_k||_F  (un-squared Frobenius norms)."""
    total = 0
    for emb in args:
        total = total + (_FrobNorm.apply(emb) if emb.dim() == 2 and emb.is_cuda and emb.dtype == torch.float32 and emb.shape[0] > 0 else torch.norm(emb, p=2))
    return total * reg


def bpr_l2_loss(user_emb, pos_item_emb, neg_item_emb, reg):
    """bpr_loss(u,p,n) + l2_reg_loss(reg,u,p) in one fused forward and one fused backward kernel."""
    return _BprL2Rows.apply(user_emb, pos_item_emb, neg_item_emb, float(reg), 'both')


class _AdvBprRows(torch.autograd.Function):
    """APR's adversarial BPR term on already-gathered [B,d] rows (fused kernel over a packed copy); the kernel computes the loss and its gradient
    in the forward call, the backward scales it."""

    @staticmethod
    def forward(ctx, user_emb, pos_emb, neg_emb, eps, groups):
        B = user_emb.shape[0]
        packed = torch.cat([user_emb, pos_emb, neg_emb], 0).contiguous()
        ar = torch.arange(B, dtype=torch.int32, device=packed.device)
        G = torch.zeros_like(packed) if any(ctx.needs_input_grad[:3]) else None
        out = ops.bpr_adv_fwd_bwd(packed, B, ar, ar, ar + B, eps, groups=groups, G=G, check_range=False, distinct_rows=True)
        ctx.B = B
        ctx.save_for_backward(G)
        return out[0].clone()

    @staticmethod
    def backward(ctx, gout):
        (G,) = ctx.saved_tensors
        B = ctx.B
        G = G * gout
        return G[:B], G[B:2 * B], G[2 * B:], None, None


def _bpr_composed(u, p, n):
    return torch.mean(-torch.log(10e-8 + torch.sigmoid(torch.mul(u, p).sum(dim=1) - torch.mul(u, n).sum(dim=1))))


def _adv_delta_composed(user_emb, pos_emb, neg_emb, eps, groups):
    """The perturbation of every row of cat(user_emb, pos_emb, neg_emb), [3B, d], detached: the clean BPR's gradient per position by autograd,
    summed per group and normalised row-wise."""
    B = user_emb.shape[0]
    with torch.enable_grad():
        rows = torch.cat([user_emb, pos_emb, neg_emb], 0).detach().requires_grad_(True)
        (gamma,) = torch.autograd.grad(_bpr_composed(rows[:B], rows[B:2 * B], rows[2 * B:]), rows)
    if groups is not None:
        _, inv = torch.unique(groups.to(gamma.device), return_inverse=True)
        gamma = torch.zeros(int(inv.max()) + 1, gamma.shape[1], dtype=gamma.dtype, device=gamma.device).index_add_(0, inv, gamma)[inv]
    return eps * gamma * torch.rsqrt(torch.clamp((gamma * gamma).sum(dim=1, keepdim=True), min=1e-12))


def _adv_bpr_composed(user_emb, pos_emb, neg_emb, eps, groups):
    """adv_bpr_loss from torch ops, any device and dtype: BPR on the rows moved by _adv_delta_composed."""
    B = user_emb.shape[0]
    delta = _adv_delta_composed(user_emb, pos_emb, neg_emb, eps, groups)
    return _bpr_composed(user_emb + delta[:B], pos_emb + delta[B:2 * B], neg_emb + delta[2 * B:])


def adv_bpr_loss(user_emb, pos_emb, neg_emb, eps, groups=None):
    """APR's adversarial term (He et al., SIGIR'18; the reference has none): bpr_loss on the rows moved by delta = eps * l2_normalize(Gamma), Gamma
    the gradient of bpr_loss(user_emb, pos_emb, neg_emb) summed per node, delta a constant of the step.  groups: integer [3B], the node of each
    row of cat(user_emb, pos_emb, neg_emb) (ids >= 0); None: every row is its own node (a per-sample perturbation).  GPU fp32 rows of a shape
    ops.bpr_adv_supported covers run the fused kernel; other tensors (CPU, float64, larger batches or widths) take the same steps from torch ops."""
    B = user_emb.shape[0]
    if groups is not None:
        if groups.dim() != 1 or groups.numel() != 3 * B or groups.is_floating_point():
            raise ValueError('adv_bpr_loss: groups must be an integer tensor of length 3B = %d' % (3 * B))
    if _kernel_rows(user_emb, pos_emb, neg_emb) and user_emb.shape == pos_emb.shape == neg_emb.shape and ops.bpr_adv_supported(B, user_emb.shape[1]):
        if groups is not None:
            groups = groups.to(device=user_emb.device, dtype=torch.int32).contiguous()
        return _AdvBprRows.apply(user_emb, pos_emb, neg_emb, float(eps), groups)
    return _adv_bpr_composed(user_emb, pos_emb, neg_emb, eps, groups)


class _WrmfL2Rows(torch.autograd.Function):
    """wrmf_loss(u,p,n) [+ reg*(||u||_F+||p||_F)] on already-gathered [B,d] rows (fused kernel over a packed copy)."""

    @staticmethod
    def forward(ctx, user_emb, pos_emb, neg_emb, reg, pos_weight):
        B, d = user_emb.shape
        packed = torch.cat([user_emb, pos_emb, neg_emb], 0).contiguous()
        ar = torch.arange(B, dtype=torch.int32, device=packed.device)
        out = ops.wrmf_l2_fwd_bwd(packed, B, ar, ar, ar + B, reg, pos_weight, None, check_range=False)
        ctx.save_for_backward(packed)
        ctx.reg, ctx.pos_weight, ctx.B = reg, pos_weight, B
        return out[0] + out[1]

    @staticmethod
    def backward(ctx, gout):
        (packed,) = ctx.saved_tensors
        B = ctx.B
        ar = torch.arange(B, dtype=torch.int32, device=packed.device)
        G = torch.zeros_like(packed)
        ops.wrmf_l2_fwd_bwd(packed, B, ar, ar, ar + B, ctx.reg, ctx.pos_weight, G, upstream=1.0, check_range=False, distinct_rows=True)
        G *= gout
        return G[:B], G[B:2 * B], G[2 * B:], None, None


def _kernel_rows(*ts):
    return all(t.dim() == 2 and t.is_cuda and t.dtype == torch.float32 and t.shape[0] > 0 for t in ts)


def wrmf_loss(user_emb, pos_item_emb, neg_item_emb, pos_weight=20):
    """util/loss.py:11-15: sum_b pos_weight (<u,p> - 1)^2 + <u,n>^2 -- a SUM over the batch, not a mean.  GPU fp32 rows run the fused kernel;
    other tensors (CPU, float64) take the reference's own expression."""
    if _kernel_rows(user_emb, pos_item_emb, neg_item_emb):
        return _WrmfL2Rows.apply(user_emb, pos_item_emb, neg_item_emb, 0.0, float(pos_weight))
    pos_score = torch.mul(user_emb, pos_item_emb).sum(dim=1)
    neg_score = torch.mul(user_emb, neg_item_emb).sum(dim=1)
    return (pos_weight * ((pos_score - 1) ** 2) + (neg_score - 0) ** 2).sum()


def wrmf_l2_loss(user_emb, pos_item_emb, neg_item_emb, reg, pos_weight=20):
    """wrmf_loss(u,p,n) + l2_reg_loss(reg,u,p) (recommender/WRMF.py:42-43) in one fused forward and one fused backward kernel."""
    return _WrmfL2Rows.apply(user_emb, pos_item_emb, neg_item_emb, float(reg), float(pos_weight))


class _InfoNCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, view1, view2, temperature):
        v1, v2 = view1.contiguous(), view2.contiguous()
        loss, d1, d2 = ops.infonce_fwd_bwd(v1, v2, float(temperature), want_grad=True)
        ctx.save_for_backward(d1, d2)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gout):
        d1, d2 = ctx.saved_tensors
        return d1 * gout, d2 * gout, None


def InfoNCE(view1, view2, temperature):
    """util/loss.py:42-49."""
    return _InfoNCE.apply(view1, view2, temperature)


def batch_softmax_loss(user_emb, item_emb, temperature):
    """util/loss.py:32-39: the arithmetic of InfoNCE (:42-49) under other argument names -- GPU fp32 rows run the same kernel within the same limits;
    other tensors (CPU, float64) take the reference's own expression."""
    if _kernel_rows(user_emb, item_emb):
        return _InfoNCE.apply(user_emb, item_emb, temperature)
    user_emb, item_emb = F.normalize(user_emb, dim=1), F.normalize(item_emb, dim=1)
    pos = torch.exp((user_emb * item_emb).sum(dim=-1) / temperature)
    ttl = torch.exp(torch.matmul(user_emb, item_emb.transpose(0, 1)) / temperature).sum(dim=1)
    return torch.mean(-torch.log(pos / ttl))


class _Alignment(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, alpha):
        loss, dx, dy = pairloss.alignment(x.contiguous(), y.contiguous(), alpha, want_grad=True)
        ctx.save_for_backward(dx, dy)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gout):
        dx, dy = ctx.saved_tensors
        return (dx * gout if ctx.needs_input_grad[0] else None), (dy * gout if ctx.needs_input_grad[1] else None), None


def alignment_loss(x, y, alpha=2):
    """util/loss.py:17-19: mean_b ||normalize(x_b) - normalize(y_b)||^alpha.  GPU fp32 rows of a width the kernel covers run it (forward and both
    gradients in one launch); other tensors (CPU, float64, other widths) take the reference's own expression."""
    if _kernel_rows(x, y) and x.shape == y.shape and x.shape[1] % 4 == 0 and x.shape[1] <= pairloss.ALIGNMENT_MAX_WIDTH and x.shape[0] <= pairloss.PAIRLOSS_MAX_ROWS:
        if not (torch.is_grad_enabled() and (x.requires_grad or y.requires_grad)):      # nobody will ask for the gradients: the forward launch alone
            return pairloss.alignment(x.contiguous(), y.contiguous(), alpha, want_grad=False)[0][0].clone()
        return _Alignment.apply(x, y, alpha)
    x, y = F.normalize(x, dim=-1), F.normalize(y, dim=-1)
    return (x - y).norm(p=2, dim=1).pow(alpha).mean()


class _Uniformity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t):
        loss, dx = pairloss.uniformity(x.contiguous(), t, want_grad=True)
        ctx.save_for_backward(dx)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gout):
        (dx,) = ctx.saved_tensors
        return dx * gout, None


def uniformity_loss(x, t=2):
    """util/loss.py:21-23: log mean_{i<j} exp(-t ||normalize(x_i) - normalize(x_j)||^2).  GPU fp32 rows of a width in pairloss.PAIRLOSS_WIDTHS, at
    least two of them, run the streaming kernel (no pairwise-distance array); other tensors (CPU, float64, other widths, fewer than two rows -- where
    the reference returns NaN) take the reference's own expression."""
    if _kernel_rows(x) and x.shape[1] in pairloss.PAIRLOSS_WIDTHS and 2 <= x.shape[0] <= pairloss.PAIRLOSS_MAX_ROWS:
        if not (torch.is_grad_enabled() and x.requires_grad):      # a diagnostic (no_grad, detached rows): half the work, no partial-tile workspace
            return pairloss.uniformity(x.contiguous(), t, want_grad=False)[0][0].clone()
        return _Uniformity.apply(x, t)
    return torch.pdist(F.normalize(x, dim=-1), p=2).pow(2).mul(-t).exp().mean().log()


def _kl_rows(a_logit, b_logit):
    return torch.sum(F.softmax(a_logit, dim=-1) * (F.log_softmax(a_logit, dim=-1) - F.log_softmax(b_logit, dim=-1)), 1)


def kl_divergence(p_logit, q_logit):
    """util/loss.py:52-55: mean over rows of KL(softmax(p) || softmax(q)).  The reference's expression composed from torch ops: no model's path calls
    it, so it has no kernel."""
    return torch.mean(_kl_rows(p_logit, q_logit))


def js_divergence(p_logit, q_logit):
    """util/loss.py:57-62: mean over rows of KL(p || q) + KL(q || p) (the reference's symmetrised sum, not halved).  Composed from torch ops like
    kl_divergence."""
    return torch.mean(_kl_rows(p_logit, q_logit) + _kl_rows(q_logit, p_logit))

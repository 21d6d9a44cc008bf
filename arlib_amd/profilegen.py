"""GSPAttack's profile generator (csrc/arl_profilegen.hip; reference attack/Black/GSPAttack.py:120-130, 201-202, 224-231) as tensor-level ops: the
pair-MLP head over every (fake user, item) pair and the relaxed Gumbel top-k over its logits -- the kernels as autograd functions, the composed
torch routes past their limits, and the dispatchers.  Re-exported by arlib_amd.ops; the limits below are read from THIS module.

    x[f, i] = b2 + sum_h w2[h] relu(A[f, h] + B[i, h]),     A = E_f W1[:, :d]^T + b1,  B = E_i W1[:, d:]^T     (the two GEMMs stay the caller's)
    round r, over the items not picked before:  z = (x + g_r) / tau,  y_r = softmax(z),  j_r = argmax z;     S = sum_r y_r
"""
import torch
from torch.utils.checkpoint import checkpoint

from . import _lib
from ._lib import check


def _ops():
    from . import ops
    return ops


PAIR_MLP_MAX_H = 1024                          # hidden width of the pair-MLP kernels (H = int(sqrt(I)): 41 on ml-100k, 316 at cfg2)
PAIR_MLP_MAX_F = 8 * 65535                     # fake users: 8 per workgroup on the grid's second axis
GUMBEL_MAX_K = 512                             # rounds: the per-round statistics of a row sit in LDS
PROFILE_MAX_I = 2 ** 31 - 1 - 2048             # items: the kernels' item index arithmetic stays in int32
GRID_MAX = 2 ** 31 - 1                         # workgroups on the grid's first axis
COMPOSED_CHUNK_ELEMS = 2 ** 24                 # the composed pair MLP keeps chunk x I x H activations under this many elements


# ------------------------------------------------------------------------------------------------ pair-MLP head
def pair_mlp_supported(F, I, H):
    """True when the pair-MLP kernels take the shape; everything else goes through pair_mlp_logits_composed."""
    F, I, H = int(F), int(I), int(H)
    return 1 <= H <= PAIR_MLP_MAX_H and 1 <= F <= PAIR_MLP_MAX_F and 1 <= I <= PROFILE_MAX_I


def _pair_args(A, B, w2, b2, what):
    o = _ops()
    o._dev(A, torch.float32, 'A', 2); o._dev(B, torch.float32, 'B', 2); o._dev(w2, torch.float32, 'w2', 1); o._dev(b2, torch.float32, 'b2')
    (F, H), I = A.shape, B.shape[0]
    if B.shape[1] != H or w2.numel() != H or b2.numel() != 1 or F == 0 or I == 0 or H == 0:
        raise ValueError('%s: A [F, H], B [I, H], w2 [H] and b2 [1] with F, I, H >= 1' % what)
    if not pair_mlp_supported(F, I, H):
        raise ValueError('%s: F = %d, I = %d, H = %d outside the kernels\' limits (H <= %d, F <= %d): use pair_mlp_logits_composed'
                         % (what, F, I, H, PAIR_MLP_MAX_H, PAIR_MLP_MAX_F))
    return F, I, H


def pair_mlp_fwd(A, B, w2, b2):
    """The forward kernel: x [F, I] for A [F, H], B [I, H], w2 [H], b2 [1], fp32 device tensors.  No autograd."""
    F, I, H = _pair_args(A, B, w2, b2, 'pair_mlp_fwd')
    x = torch.empty(F, I, dtype=torch.float32, device=A.device)
    _ptr = _ops()._ptr
    check(_lib.lib().arl_pair_mlp_fwd_f32(_ptr(A), F, _ptr(B), I, H, _ptr(w2), _ptr(b2), _ptr(x), _ops()._stream()), 'arl_pair_mlp_fwd_f32')
    return x


def pair_mlp_bwd(g, A, B, w2, b2):
    """The backward kernels for an upstream g [F, I]: (dA [F, H], dB [I, H], dw2 [H], db2 [1]).  The ReLU derivative at exactly 0 is 0."""
    F, I, H = _pair_args(A, B, w2, b2, 'pair_mlp_bwd')
    _ops()._dev(g, torch.float32, 'g', 2)
    if tuple(g.shape) != (F, I):
        raise ValueError('pair_mlp_bwd: g [F, I]')
    L, _ptr, dev = _lib.lib(), _ops()._ptr, A.device
    ws = torch.empty(max(L.arl_pair_mlp_workspace_bytes(F, I, H), 16), dtype=torch.uint8, device=dev)
    dA, dB, dw2, db2 = torch.empty_like(A), torch.empty_like(B), torch.empty_like(w2), torch.empty(1, dtype=torch.float32, device=dev)
    check(L.arl_pair_mlp_bwd_f32(_ptr(g), _ptr(A), F, _ptr(B), I, H, _ptr(w2), _ptr(dA), _ptr(dB), _ptr(dw2), _ptr(db2), _ptr(ws), _ops()._stream()),
          'arl_pair_mlp_bwd_f32')
    return dA, dB, dw2, db2


class _PairMlp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, A, B, w2, b2):
        A, B, w2, b2 = A.contiguous(), B.contiguous(), w2.contiguous(), b2.contiguous()
        ctx.save_for_backward(A, B, w2, b2)
        return pair_mlp_fwd(A, B, w2, b2)

    @staticmethod
    def backward(ctx, g):
        A, B, w2, b2 = ctx.saved_tensors
        dA, dB, dw2, db2 = pair_mlp_bwd(g.contiguous(), A, B, w2, b2)
        return dA, dB, dw2, db2.view(b2.shape)


def pair_mlp_logits(A, B, w2, b2):
    """x [F, I] = b2 + sum_h w2[h] relu(A[f, h] + B[i, h]) on the kernels, differentiable in all four.  Shapes outside pair_mlp_supported raise."""
    _pair_args(A, B, w2, b2, 'pair_mlp_logits')
    return _PairMlp.apply(A, B, w2, b2)


def pair_mlp_logits_composed(A, B, w2, b2, chunk=None):
    """The same logits composed from torch ops (any dtype, CPU or GPU), `chunk` fake users at a time and recomputed in the backward, so at most
    chunk x I x H activations exist: the route past the kernels' limits and the yardstick of the tests and tools/gsp_bench.py."""
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1] or w2.numel() != A.shape[1] or b2.numel() != 1:
        raise ValueError('pair_mlp_logits_composed: A [F, H], B [I, H], w2 [H] and b2 [1]')
    (F, H), I = A.shape, B.shape[0]
    if chunk is None:
        chunk = max(1, COMPOSED_CHUNK_ELEMS // max(1, I * H))

    def panel(a, Bm, w, b):
        return torch.relu(a[:, None, :] + Bm[None]) @ w.reshape(-1) + b.reshape(())
    rows = [checkpoint(panel, A[f:f + chunk], B, w2, b2, use_reentrant=False) for f in range(0, F, chunk)]
    return rows[0] if len(rows) == 1 else torch.cat(rows, 0)


def pair_mlp_logits_auto(A, B, w2, b2):
    """pair_mlp_logits where the kernels take the shape, pair_mlp_logits_composed otherwise."""
    if pair_mlp_supported(A.shape[0], B.shape[0], A.shape[1]):
        return pair_mlp_logits(A, B, w2, b2)
    _ops()._dev(A, torch.float32, 'A', 2)
    return pair_mlp_logits_composed(A, B, w2, b2)


# ------------------------------------------------------------------------------------------------ relaxed Gumbel top-k
def gumbel_topk_supported(F, I, k):
    """True when the Gumbel top-k kernels take the shape; everything else goes through gumbel_topk_composed."""
    F, I, k = int(F), int(I), int(k)
    return 1 <= k <= min(I, GUMBEL_MAX_K) and 1 <= I <= PROFILE_MAX_I and 1 <= F and F * ((I + 255) // 256) <= GRID_MAX


def gumbel_noise_supported(k, F, I):
    k, F, I = int(k), int(F), int(I)
    return 1 <= k <= GUMBEL_MAX_K and 1 <= I <= PROFILE_MAX_I and 1 <= F and k * F * ((I + 255) // 256) <= GRID_MAX


def gumbel_noise(seed, call, k, F, I, device='cuda'):
    """The counter-hash Gumbel draw as a tensor [k, F, I]: the value at (r, f, i) depends on (seed, call, r, f, i) only, and is what
    gumbel_topk(..., seed=seed, call=call) uses without storing it."""
    k, F, I = int(k), int(F), int(I)
    if not gumbel_noise_supported(k, F, I):
        raise ValueError('gumbel_noise: 1 <= k <= %d, F, I >= 1 and k F ceil(I / 256) < 2^31' % GUMBEL_MAX_K)
    if torch.device(device).type != 'cuda':
        raise _lib.ArlError('gumbel_noise: the device must be the GPU (no CPU fallback in arlib_amd)')
    g = torch.empty(k, F, I, dtype=torch.float32, device=device)
    with torch.cuda.device(g.device):
        check(_lib.lib().arl_gumbel_noise_f32(int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1), k, F, I, _ops()._ptr(g), _ops()._stream()), 'arl_gumbel_noise_f32')
    return g


def _gumbel_args(x, k, tau, noise, seed, what):
    o = _ops()
    o._dev(x, torch.float32, 'x', 2)
    F, I = x.shape
    k = int(k)
    if F == 0 or not 1 <= k <= I or not float(tau) > 0:
        raise ValueError('%s: x [F, I] with F >= 1, 1 <= k <= I and tau > 0' % what)
    if (noise is None) == (seed is None):
        raise ValueError('%s: exactly one of noise and seed' % what)
    if noise is not None:
        o._dev(noise, torch.float32, 'noise', 3)
        if tuple(noise.shape) != (k, F, I):
            raise ValueError('%s: noise [k, F, I]' % what)
    if not gumbel_topk_supported(F, I, k):
        raise ValueError('%s: F = %d, I = %d, k = %d outside the kernels\' limits (k <= %d): use gumbel_topk_composed' % (what, F, I, k, GUMBEL_MAX_K))
    return F, I, k


def _seed_call(seed, call):
    return (0, 0) if seed is None else (int(seed) & (2 ** 64 - 1), int(call) & (2 ** 64 - 1))


def gumbel_topk_fwd(x, k, tau=1.0, noise=None, seed=None, call=0):
    """The forward kernels: (S [F, I], picks [F, k] int32, logsumexp [F, k], stats [F, k, 2] = every round's (max, sum)).  No autograd."""
    F, I, k = _gumbel_args(x, k, tau, noise, seed, 'gumbel_topk_fwd')
    L, _ptr, dev = _lib.lib(), _ops()._ptr, x.device
    ws = torch.empty(max(L.arl_gumbel_topk_workspace_bytes(F, I, k, 0), 16), dtype=torch.uint8, device=dev)
    S = torch.empty_like(x)
    picks, logsumexp = torch.empty(F, k, dtype=torch.int32, device=dev), torch.empty(F, k, dtype=torch.float32, device=dev)
    stats = torch.empty(F, k, 2, dtype=torch.float32, device=dev)
    s, c = _seed_call(seed, call)
    check(L.arl_gumbel_topk_fwd_f32(_ptr(x), F, I, k, float(tau), _ptr(noise), s, c, _ptr(S), _ptr(picks), _ptr(logsumexp), _ptr(stats), _ptr(ws), _ops()._stream()),
          'arl_gumbel_topk_fwd_f32')
    return S, picks, logsumexp, stats


def gumbel_topk_bwd(dS, x, k, picks, stats, tau=1.0, noise=None, seed=None, call=0):
    """dx [F, I] for an upstream dS [F, I], with the argmax detached; picks and stats are gumbel_topk_fwd's, the noise source the same."""
    F, I, k = _gumbel_args(x, k, tau, noise, seed, 'gumbel_topk_bwd')
    o = _ops()
    o._dev(dS, torch.float32, 'dS', 2); o._dev(picks, torch.int32, 'picks', 2); o._dev(stats, torch.float32, 'stats', 3)
    if tuple(dS.shape) != (F, I) or tuple(picks.shape) != (F, k) or tuple(stats.shape) != (F, k, 2):
        raise ValueError('gumbel_topk_bwd: dS [F, I], picks [F, k], stats [F, k, 2]')
    L, _ptr = _lib.lib(), o._ptr
    ws = torch.empty(max(L.arl_gumbel_topk_workspace_bytes(F, I, k, 1), 16), dtype=torch.uint8, device=x.device)
    dx = torch.empty_like(x)
    s, c = _seed_call(seed, call)
    check(L.arl_gumbel_topk_bwd_f32(_ptr(x), F, I, k, float(tau), _ptr(noise), s, c, _ptr(picks), _ptr(stats), _ptr(dS), _ptr(dx), _ptr(ws), o._stream()),
          'arl_gumbel_topk_bwd_f32')
    return dx


class _GumbelTopk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, tau, noise, seed, call):
        x = x.contiguous()
        S, picks, _, stats = gumbel_topk_fwd(x, k, tau, noise, seed, call)
        ctx.save_for_backward(x, picks, stats)                      # O(F I + F k) of its own; the noise tensor, when there is one, is the caller's
        ctx.noise, ctx.args = noise, (int(k), float(tau), seed, call)
        picks64 = picks.long()
        ctx.mark_non_differentiable(picks64)
        return S, picks64

    @staticmethod
    def backward(ctx, dS, _):
        x, picks, stats = ctx.saved_tensors
        k, tau, seed, call = ctx.args
        return gumbel_topk_bwd(dS.contiguous(), x, k, picks, stats, tau, ctx.noise, seed, call), None, None, None, None, None


def gumbel_topk(x, k, tau=1.0, noise=None, seed=None, call=0):
    """Relaxed k-hot rows on the kernels, GSPAttack.gumbel_topk_relaxed's semantics: (S [F, I], picks [F, k] int64), differentiable in x with the
    argmax detached.  Exactly one of noise [k, F, I] and seed (the counter hash of (seed, call, r, f, i); no [k, F, I] tensor exists)."""
    _gumbel_args(x, k, tau, noise, seed, 'gumbel_topk')
    if noise is not None:
        noise = noise.detach()
    return _GumbelTopk.apply(x, int(k), float(tau), noise, seed, call)


def gumbel_topk_composed(x, k, tau=1.0, noise=None, seed=None, call=0):
    """The same on GSPAttack.gumbel_topk_relaxed (k rounds of torch ops); with a seed the hash draw is written out first (gumbel_noise, which
    covers GUMBEL_MAX_K rounds: more rounds than that need a noise tensor)."""
    from .attack.Black.GSPAttack import gumbel_topk_relaxed
    if (noise is None) == (seed is None):
        raise ValueError('gumbel_topk_composed: exactly one of noise and seed')
    if noise is None:
        noise = gumbel_noise(seed, call, k, x.shape[0], x.shape[1], x.device)
    return gumbel_topk_relaxed(x, int(k), tau=tau, noise=noise)


def gumbel_topk_auto(x, k, tau=1.0, noise=None, seed=None, call=0):
    """gumbel_topk where the kernels take the shape, gumbel_topk_composed otherwise."""
    if x.dim() == 2 and gumbel_topk_supported(x.shape[0], x.shape[1], k):
        return gumbel_topk(x, k, tau, noise, seed, call)
    _ops()._dev(x, torch.float32, 'x', 2)
    return gumbel_topk_composed(x, k, tau, noise, seed, call)

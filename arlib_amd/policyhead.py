"""PoisonRec's policy head (csrc/arl_policyhead.hip; reference attack/Black/PoisonRec.py:363-371, 398-401) as tensor-level ops: a Bernoulli
distribution over every item whose logits are the softmax probabilities of z = q E^T [B, I] -- the streaming kernels, the composed torch routes past
their limits, the dispatchers and the autograd function.  Re-exported by arlib_amd.ops; the limits below are read from THIS module.

With p = softmax_i(z), sp = softplus(p), sg = sigmoid(p) and action bits a:
    logp[b] = sum_i (a p - sp),     ent[b] = sum_i (sp - p sg),
and dq, dE are the gradients of sum_b gl[b] logp[b] + ge[b] ent[b].  Actions travel packed: [B, ceil(I / 32)] int32, bit i % 32 of word i / 32 is
item i, pad bits 0.  Sampling sets a_i = (u_i < sg_i); the deterministic mode picks a_i = (p_i > 0), which is sg_i > 1/2."""
import torch

from . import _lib
from ._lib import check


def _ops():
    from . import ops
    return ops


POLICYHEAD_WIDTHS = (16, 32, 64, 128)
POLICYHEAD_MAX_ROWS = (2 ** 31 - 1) // 128     # rows of either table: every row * d offset of the kernel's index arithmetic stays in int32
POLICYHEAD_CHUNK_ELEMS = 2 ** 24               # the composed routes keep their row panels under this many elements
_M64 = 2 ** 64 - 1


def bernoulli_softmax_supported(B, I, d):
    """True when the streaming kernels take the shape; everything else goes through the composed routes."""
    B, I, d = int(B), int(I), int(d)
    return d in POLICYHEAD_WIDTHS and 1 <= B <= POLICYHEAD_MAX_ROWS and 1 <= I <= POLICYHEAD_MAX_ROWS


# ------------------------------------------------------------------------------------------------ packed actions
def pack_bits(a):
    """[B, I] of zeros and non-zeros (any dtype) -> [B, ceil(I / 32)] int32, bit i % 32 of word i / 32 = item i, pad bits 0.  CPU or GPU."""
    if a.dim() != 2:
        raise ValueError('pack_bits: a [B, I]')
    B, I = a.shape
    W = (I + 31) // 32
    bits = torch.zeros(B, W * 32, dtype=torch.int64, device=a.device)
    bits[:, :I] = (a != 0).to(torch.int64)
    w = (bits.view(B, W, 32) << torch.arange(32, dtype=torch.int64, device=a.device)).sum(2)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def unpack_bits(words, I):
    """[B, W] int32 -> [B, I] bool; the inverse of pack_bits (pad bits are dropped)."""
    I = int(I)
    if words.dim() != 2 or words.dtype != torch.int32 or words.shape[1] != (I + 31) // 32:
        raise ValueError('unpack_bits: words [B, ceil(I / 32)] int32')
    w = words.to(torch.int64) & 0xFFFFFFFF
    bits = (w[:, :, None] >> torch.arange(32, dtype=torch.int64, device=words.device)) & 1
    return bits.view(words.shape[0], -1)[:, :I].bool()


def _panel_rows(I, chunk):
    return max(1, POLICYHEAD_CHUNK_ELEMS // max(1, int(I))) if chunk is None else max(1, int(chunk))


def _head_shapes(q, E, what):
    if q.dim() != 2 or E.dim() != 2 or q.shape[1] != E.shape[1] or q.shape[0] == 0 or E.shape[0] == 0:
        raise ValueError('%s: q [B, d] and E [I, d] with B, I >= 1' % what)
    return q.shape[0], E.shape[0], q.shape[1]


def _check_actions(actions, B, I, what):
    if actions.dtype != torch.int32 or tuple(actions.shape) != (B, (I + 31) // 32):
        raise ValueError('%s: actions [B, ceil(I / 32)] int32 (pack_bits)' % what)


def _kernel_args(q, E, what):
    o = _ops()
    o._dev(q, torch.float32, 'q', 2); o._dev(E, torch.float32, 'E', 2)
    B, I, d = _head_shapes(q, E, what)
    if not bernoulli_softmax_supported(B, I, d):
        raise ValueError('%s: B = %d, I = %d, d = %d outside the kernels\' limits (d in %s, rows <= %d): use the composed route'
                         % (what, B, I, d, POLICYHEAD_WIDTHS, POLICYHEAD_MAX_ROWS))
    return B, I, d


def _workspace(B, I, d, want_grad, dev):
    return torch.empty(max(_lib.lib().arl_bernoulli_softmax_workspace_bytes(B, I, d, 1 if want_grad else 0), 16), dtype=torch.uint8, device=dev)


# ------------------------------------------------------------------------------------------------ evaluation
def bernoulli_softmax_eval(q, E, actions, gl=None, ge=None, want_grad=False):
    """The streaming kernels.  q [B, d], E [I, d] fp32 device tensors, actions packed.  Returns (logp [B], ent [B]), with want_grad
    (logp, ent, dq, dE), the gradients of sum_b gl[b] logp[b] + ge[b] ent[b] (gl, ge [B] fp32).  Shapes outside bernoulli_softmax_supported raise."""
    B, I, d = _kernel_args(q, E, 'bernoulli_softmax_eval')
    o = _ops()
    o._dev(actions, torch.int32, 'actions', 2)
    _check_actions(actions, B, I, 'bernoulli_softmax_eval')
    if want_grad:
        if gl is None or ge is None:
            raise ValueError('bernoulli_softmax_eval: gradients need the upstreams gl and ge')
        o._dev(gl, torch.float32, 'gl', 1); o._dev(ge, torch.float32, 'ge', 1)
        if gl.numel() != B or ge.numel() != B:
            raise ValueError('bernoulli_softmax_eval: gl [B], ge [B]')
    else:
        gl = ge = None
    L, _ptr, dev = _lib.lib(), o._ptr, q.device
    ws = _workspace(B, I, d, want_grad, dev)
    logp, ent = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.float32, device=dev)
    dq, dE = (torch.empty_like(q), torch.empty_like(E)) if want_grad else (None, None)
    check(L.arl_bernoulli_softmax_eval_f32(_ptr(q), B, _ptr(E), I, d, _ptr(actions), _ptr(gl), _ptr(ge), _ptr(logp), _ptr(ent), _ptr(dq), _ptr(dE), _ptr(ws),
                                           o._stream()), 'arl_bernoulli_softmax_eval_f32')
    return (logp, ent, dq, dE) if want_grad else (logp, ent)


def bernoulli_softmax_eval_composed(q, E, actions, gl=None, ge=None, want_grad=False, chunk=None):
    """The same quantities composed from torch ops in the tensors' dtype (fp32 in the product), in row panels of `chunk` rows: the route past the
    kernels' limits, the only route on the CPU, and the yardstick of the tests and tools/poisonrec_bench.py.  Peak memory: a few chunk x I panels."""
    B, I, d = _head_shapes(q, E, 'bernoulli_softmax_eval_composed')
    _check_actions(actions, B, I, 'bernoulli_softmax_eval_composed')
    if want_grad and (gl is None or ge is None):
        raise ValueError('bernoulli_softmax_eval_composed: gradients need the upstreams gl and ge')
    rows = _panel_rows(I, chunk)
    logp, ent = torch.empty(B, dtype=q.dtype, device=q.device), torch.empty(B, dtype=q.dtype, device=q.device)
    dq, dE = (torch.empty_like(q), torch.zeros_like(E)) if want_grad else (None, None)
    for b in range(0, B, rows):
        e = min(B, b + rows)
        a = unpack_bits(actions[b:e], I).to(q.dtype)
        p = torch.softmax(q[b:e] @ E.t(), dim=1)
        sp, sg = torch.nn.functional.softplus(p), torch.sigmoid(p)
        logp[b:e] = (a * p - sp).sum(1)
        ent[b:e] = (sp - p * sg).sum(1)
        if want_grad:
            c = gl[b:e, None] * (a - sg) - ge[b:e, None] * (p * sg * (1 - sg))
            dz = p * (c - (p * c).sum(1, keepdim=True))
            dq[b:e] = dz @ E
            dE += dz.t() @ q[b:e]
    return (logp, ent, dq, dE) if want_grad else (logp, ent)


def bernoulli_softmax(q, E, actions, gl=None, ge=None, want_grad=False):
    """bernoulli_softmax_eval where the kernels take the shape, bernoulli_softmax_eval_composed otherwise."""
    if q.dim() == 2 and E.dim() == 2 and bernoulli_softmax_supported(q.shape[0], E.shape[0], q.shape[1]):
        return bernoulli_softmax_eval(q, E, actions, gl, ge, want_grad)
    _ops()._dev(q, torch.float32, 'q', 2)
    return bernoulli_softmax_eval_composed(q, E, actions, gl, ge, want_grad)


class _BernoulliSoftmaxHead(torch.autograd.Function):
    """(logp, ent) of the head; the backward runs the gradient passes with the two upstreams and feeds dq and dE into the graph.  Saved: q, E and the
    packed actions -- O(B + I) rows, no B x I tensor."""

    @staticmethod
    def forward(ctx, q, E, actions, fused):
        q, E = q.contiguous(), E.contiguous()
        ctx.save_for_backward(q, E, actions)
        ctx.fused = fused
        logp, ent = (bernoulli_softmax_eval if fused else bernoulli_softmax_eval_composed)(q, E, actions)
        return logp, ent

    @staticmethod
    def backward(ctx, gl, ge):
        q, E, actions = ctx.saved_tensors
        gl = torch.zeros(q.shape[0], dtype=q.dtype, device=q.device) if gl is None else gl.contiguous()
        ge = torch.zeros(q.shape[0], dtype=q.dtype, device=q.device) if ge is None else ge.contiguous()
        _, _, dq, dE = (bernoulli_softmax_eval if ctx.fused else bernoulli_softmax_eval_composed)(q, E, actions, gl, ge, want_grad=True)
        return dq, dE, None, None


def bernoulli_softmax_head(q, E, actions, route='auto'):
    """(logp [B], ent [B]) differentiable in q and E.  route 'fused': the kernels (shapes outside their limits raise); 'composed': torch, CPU or GPU;
    'auto': the kernels on a GPU where they take the shape."""
    if route not in ('auto', 'fused', 'composed'):
        raise ValueError("bernoulli_softmax_head: route is 'auto', 'fused' or 'composed', not %r" % (route,))
    B, I, d = _head_shapes(q, E, 'bernoulli_softmax_head')
    if route == 'auto':
        route = 'fused' if q.is_cuda and q.dtype == torch.float32 and bernoulli_softmax_supported(B, I, d) else 'composed'
    if route == 'fused':
        _kernel_args(q.detach().contiguous(), E.detach().contiguous(), 'bernoulli_softmax_head')
    _check_actions(actions, B, I, 'bernoulli_softmax_head')
    return _BernoulliSoftmaxHead.apply(q, E, actions, route == 'fused')


# ------------------------------------------------------------------------------------------------ sampling
def bernoulli_uniforms(seed, call, B, I, row0=0, device='cuda'):
    """The counter-hash draw as a tensor [B, I] in [0, 1): the value at (b, i) depends on (seed, call, row0 + b, i) only, and is what
    bernoulli_softmax_sample(..., seed=seed, call=call, row0=row0) uses without storing it."""
    B, I, row0 = int(B), int(I), int(row0)
    if B < 1 or I < 1 or row0 < 0 or I > 2 ** 31 - 1 - 256 or row0 + B > 2 ** 31 - 1 or B * ((I + 255) // 256) > 2 ** 31 - 1:
        raise ValueError('bernoulli_uniforms: B, I >= 1, row0 >= 0 and B ceil(I / 256) < 2^31')
    if torch.device(device).type != 'cuda':
        raise _lib.ArlError('bernoulli_uniforms: the device must be the GPU (no CPU fallback in arlib_amd)')
    u = torch.empty(B, I, dtype=torch.float32, device=device)
    with torch.cuda.device(u.device):
        check(_lib.lib().arl_bernoulli_uniforms_f32(int(seed) & _M64, int(call) & _M64, row0, B, I, _ops()._ptr(u), _ops()._stream()), 'arl_bernoulli_uniforms_f32')
    return u


def _sample_args(B, I, u, seed, deterministic, what):
    if deterministic:
        if u is not None or seed is not None:
            raise ValueError('%s: the deterministic mode takes neither u nor seed' % what)
    elif (u is None) == (seed is None):
        raise ValueError('%s: exactly one of u and seed' % what)
    if u is not None and tuple(u.shape) != (B, I):
        raise ValueError('%s: u [B, I]' % what)


def bernoulli_softmax_sample(q, E, u=None, seed=None, call=0, row0=0, deterministic=False):
    """The sampling kernels: (actions [B, W] int32 packed, logp [B], count [B] int32 the set bits per row).  a_i = (u_i < sg_i) with u the caller's
    [B, I] fp32 tensor or, with a seed, the counter hash of (seed, call, row0 + b, i) (no [B, I] tensor exists); deterministic: a_i = (p_i > 0)."""
    B, I, d = _kernel_args(q, E, 'bernoulli_softmax_sample')
    _sample_args(B, I, u, seed, deterministic, 'bernoulli_softmax_sample')
    o = _ops()
    if u is not None:
        o._dev(u, torch.float32, 'u', 2)
    row0 = int(row0)
    if row0 < 0 or row0 + B > 2 ** 31 - 1:
        raise ValueError('bernoulli_softmax_sample: 0 <= row0 and row0 + B < 2^31')
    L, _ptr, dev = _lib.lib(), o._ptr, q.device
    ws = _workspace(B, I, d, False, dev)
    actions = torch.empty(B, (I + 31) // 32, dtype=torch.int32, device=dev)
    logp, count = torch.empty(B, dtype=torch.float32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
    s, c = (0, 0) if seed is None else (int(seed) & _M64, int(call) & _M64)
    check(L.arl_bernoulli_softmax_sample_f32(_ptr(q), B, _ptr(E), I, d, _ptr(u), s, c, row0, 1 if deterministic else 0, _ptr(actions), _ptr(logp), _ptr(count),
                                             _ptr(ws), o._stream()), 'arl_bernoulli_softmax_sample_f32')
    return actions, logp, count


def bernoulli_softmax_sample_composed(q, E, u=None, seed=None, call=0, row0=0, deterministic=False, chunk=None):
    """The same composed from torch ops, in row panels; with a seed the hash draw is written out first (bernoulli_uniforms, GPU only)."""
    B, I, d = _head_shapes(q, E, 'bernoulli_softmax_sample_composed')
    _sample_args(B, I, u, seed, deterministic, 'bernoulli_softmax_sample_composed')
    rows = _panel_rows(I, chunk)
    actions = torch.empty(B, (I + 31) // 32, dtype=torch.int32, device=q.device)
    logp, count = torch.empty(B, dtype=q.dtype, device=q.device), torch.empty(B, dtype=torch.int32, device=q.device)
    for b in range(0, B, rows):
        e = min(B, b + rows)
        p = torch.softmax(q[b:e] @ E.t(), dim=1)
        sg = torch.sigmoid(p)
        if deterministic:
            a = p > 0
        else:
            uu = u[b:e] if u is not None else bernoulli_uniforms(seed, call, e - b, I, int(row0) + b, q.device)
            a = uu.to(q.dtype) < sg
        actions[b:e] = pack_bits(a)
        logp[b:e] = (a.to(q.dtype) * p - torch.nn.functional.softplus(p)).sum(1)
        count[b:e] = a.sum(1).to(torch.int32)
    return actions, logp, count


def bernoulli_softmax_sample_auto(q, E, u=None, seed=None, call=0, row0=0, deterministic=False):
    """bernoulli_softmax_sample where the kernels take the shape, bernoulli_softmax_sample_composed otherwise."""
    if q.dim() == 2 and E.dim() == 2 and q.is_cuda and q.dtype == torch.float32 and bernoulli_softmax_supported(q.shape[0], E.shape[0], q.shape[1]):
        return bernoulli_softmax_sample(q, E, u, seed, call, row0, deterministic)
    return bernoulli_softmax_sample_composed(q, E, u, seed, call, row0, deterministic)

"""No result may depend on what scratch memory held before the call (tests/poison.py).

Op level: every public entry of arlib_amd.ops that allocates with the empty family or takes a caller buffer (found by introspection of the module's
source, checked against the CASES table: a new op without an entry fails test_every_allocating_op_has_a_case) runs one ragged problem four ways --
clean twice, inside poisoned_allocations(), and with poisoned caller buffers -- and the clean result is held against float64.  Ops that are
bit-identical from clean run to clean run must be bit-identical under poison too (documented in-place operands included); the others are listed in
NOT_BITWISE with the reason and must meet their float64 bar without a NaN.  Then the "not read" contracts, the workspaces that outlive a call, and
three consecutive training steps of every engine / model step, clean against poisoned, with the engine's sparse state machine."""
import ast
import inspect
import numpy as np
import pytest
import torch
from conftest import close, rel_err, RTOL
from poison import poisoned_allocations, poison_, compare, has_nan
from test_gpu_kernels import random_graph, make_csr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-5                      # single kernels against float64 (test_gpu_width_classes.py); matrix-core kernels: RTOL, as their own tests
WIDTHS = (12, 64, 100, 256)     # one width per class of the row kernels: 4 / 16 / 32 / 64 lanes per row
MFMA_WIDTHS = (16, 64)
CALLER_PARAMS = ('out', 'workspace', 'loss_out', 'lse', 'sums_out')

# Ops whose two CLEAN runs are not bit-identical, with the reason; their poisoned runs are held to the float64 bar and must be NaN-free.
NOT_BITWISE = {}


@pytest.fixture(scope='module')
def ops():
    if not torch.cuda.is_available():
        pytest.fail('GPU tests need a GPU (run with -m gpu on the MI355X box)')
    from arlib_amd import ops as _ops
    return _ops


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def H(t):
    return t.detach().double().cpu().numpy()


def Pz(*shape, dtype=torch.float32):
    """A poisoned caller buffer."""
    return poison_(torch.zeros(*shape, dtype=dtype, device=DEV))


def randn(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen) * scale).to(DEV)


# ------------------------------------------------------------------------------------------------ the shared ragged graph
class Graph:
    """301 users x 83 items: two isolated users (empty rows), three hot items (rows far longer than the chunk of 32: the long-row plan with its
    partial workspace runs), N = 384 rows is no multiple of any tile the row kernels use once the listed rows are ragged."""

    def __init__(self, ops, blocked=False):
        rng = np.random.default_rng(5)
        self.U, self.I = 301, 83
        u, i = random_graph(rng, self.U, self.I, 6, hot_items=3, hot_deg=250, empty_users=(5, 77))
        self.rowptr, self.col, self.w, self.val = make_csr(u, i, self.U, self.I)
        self.N = self.U + self.I
        assert np.diff(self.rowptr).max() > 200 and np.diff(self.rowptr).min() == 0
        self.A = ops.CSRGraph(self.rowptr, self.col, self.val, DEV, chunk=32)
        assert self.A.n_long >= 3
        if blocked:
            self.A.enable_blocked(split=self.U, rows_per_wave=16, hub=24, col_block=64)
            assert sum(s['n_split'] for s in self.A.blocked.sets) > 0            # split rows: the plan's own [n_pieces, d] workspace
        rows = np.repeat(np.arange(self.N), np.diff(self.rowptr))
        M = torch.zeros(self.N, self.N, dtype=torch.float64)
        M[torch.from_numpy(rows), torch.from_numpy(self.col.astype(np.int64))] = torch.from_numpy(self.val.astype(np.float64))
        self.M = M.to(DEV)
        self.erow = T(rows.astype(np.int32))


_GRAPHS = {}


def graph(ops, blocked=False):
    if blocked not in _GRAPHS:
        _GRAPHS[blocked] = Graph(ops, blocked)
    return _GRAPHS[blocked]


def adam64(P, g, M, V, lr, step, b1=0.9, b2=0.999, eps=1e-8):
    M = b1 * M + (1 - b1) * g
    V = b2 * V + (1 - b2) * g * g
    P = P - lr / (1 - b1 ** step) * M / ((V / (1 - b2 ** step)).sqrt() + eps)
    return P, M, V


def spmm_inputs(g, d, seed):
    gen = torch.Generator().manual_seed(seed)
    X, Z = randn(gen, g.N, d), randn(gen, g.N, d)
    st = (randn(gen, g.N, d, scale=0.1), randn(gen, g.N, d, scale=0.01), torch.rand(g.N, d, generator=gen).to(DEV) * 1e-4)
    zf = (torch.rand(g.N, generator=gen) < 0.3).to(torch.uint8).to(DEV)
    return X, Z, st, zf


# ------------------------------------------------------------------------------------------------ cases: name -> builder(ops) -> (run(caller), ref())
# run(caller) returns a dict of results; with caller=True every buffer the op accepts is passed in, poisoned.  ref() returns float64 tensors for
# (a subset of) the same keys, or (tensor, tol) pairs.  In-place operands are cloned inside run and returned.
CASES = {}


def case(name):
    def deco(f):
        CASES[name] = f
        return f
    return deco


@case('norm_vals_coo')
def _(ops):
    g = graph(ops)
    gen = torch.Generator().manual_seed(1)
    w = (torch.rand(len(g.col), generator=gen) + 0.5).to(DEV)
    dinv = (torch.rand(g.N, generator=gen) + 0.5).to(DEV)
    col = T(g.col)
    return (lambda caller: {'val': ops.norm_vals_coo(g.erow, col, w, dinv)},
            lambda: {'val': dinv.double()[g.erow.long()] * w.double() * dinv.double()[col.long()]})


@case('norm_adj_values')
def _(ops):
    g = graph(ops)
    gen = torch.Generator().manual_seed(2)
    w = (torch.rand(len(g.col), generator=gen) + 0.5).to(DEV)
    rp, col = T(g.rowptr.astype(np.int32)), T(g.col)

    def run(caller):
        v1, d1 = ops.norm_adj_values(rp, col, w, g.N)
        v2, d2 = ops.norm_adj_values(rp, col, w, g.N, erow=g.erow)
        return {'val': v1, 'dinv': d1, 'val_coo': v2, 'dinv_coo': d2}

    def ref():
        deg = torch.zeros(g.N, dtype=torch.float64, device=DEV).index_add_(0, g.erow.long(), w.double())
        dinv = torch.where(deg > 0, deg.clamp_min(1e-300) ** -0.5, torch.zeros_like(deg))
        val = dinv[g.erow.long()] * w.double() * dinv[col.long()]
        return {'val': val, 'dinv': dinv, 'val_coo': val, 'dinv_coo': dinv}
    return run, ref


@case('spmm')
def _(ops):
    g, gb = graph(ops), graph(ops, True)
    ins = {d: spmm_inputs(g, d, 10 + d) for d in WIDTHS}
    rs = torch.rand(g.N, generator=torch.Generator().manual_seed(3)).to(DEV)

    def run(caller):
        r = {}
        for d, (X, Z, _, _) in ins.items():
            r['d%d' % d] = ops.spmm(g.A, X, 0.5, 0.25, Z, out=Pz(g.N, d) if caller else None)
            r['rs%d' % d] = ops.spmm(g.A, X, 0.5, 0.25, Z, out=Pz(g.N, d) if caller else None, row_scale=rs)
        r['blocked64'] = ops.spmm(gb.A, ins[64][0], 0.5, 0.25, ins[64][1], out=Pz(g.N, 64) if caller else None)
        return r

    def ref():
        r = {}
        for d, (X, Z, _, _) in ins.items():
            r['d%d' % d] = 0.5 * (g.M @ X.double()) + 0.25 * Z.double()
            r['rs%d' % d] = 0.5 * rs.double()[:, None] * (g.M @ X.double()) + 0.25 * Z.double()
        r['blocked64'] = r['d64']
        return r
    return run, ref


@case('spmm_layersum')
def _(ops):
    g, gb = graph(ops), graph(ops, True)
    ins = {d: spmm_inputs(g, d, 20 + d) for d in WIDTHS}

    def run(caller):
        r = {}
        for tag, A, d in [('d%d' % d, g.A, d) for d in WIDTHS] + [('blocked64', gb.A, 64)]:
            X, Z = ins[d][:2]
            S, Y = (Pz(g.N, d), Pz(g.N, d)) if caller else (torch.empty_like(X), torch.empty_like(X))
            ops.spmm_layersum(A, X, Z, S, Y)
            r['S' + tag], r['Y' + tag] = S, Y
        return r

    def ref():
        r = {}
        for tag, d in [('d%d' % d, d) for d in WIDTHS] + [('blocked64', 64)]:
            X, Z = ins[d][:2]
            r['Y' + tag] = g.M @ X.double()
            r['S' + tag] = Z.double() + r['Y' + tag]
        return r
    return run, ref


@case('spmm_adam')
def _(ops):
    g, gb = graph(ops), graph(ops, True)
    ins = {d: spmm_inputs(g, d, 30 + d) for d in WIDTHS}

    def run(caller):
        r = {}
        for tag, A, d in [('d%d' % d, g.A, d) for d in WIDTHS] + [('blocked64', gb.A, 64)]:
            X, Z, st, zf = ins[d]
            Pm, M, V = (t.clone() for t in st)
            ops.spmm_adam(A, X, 0.25, 0.5, Z * zf[:, None], Pm, M, V, 0.005, 7, zflags=zf)
            r['P' + tag], r['M' + tag], r['V' + tag] = Pm, M, V
        return r

    def ref():
        r = {}
        for tag, d in [('d%d' % d, d) for d in WIDTHS] + [('blocked64', 64)]:
            X, Z, st, zf = ins[d]
            grad = 0.25 * (g.M @ X.double()) + 0.5 * Z.double() * zf.double()[:, None]
            r['P' + tag], r['M' + tag], r['V' + tag] = adam64(st[0].double(), grad, st[1].double(), st[2].double(), 0.005, 7)
        return r
    return run, ref


def flag_inputs(g, d, seed):
    gen = torch.Generator().manual_seed(seed)
    nz = torch.randperm(g.N, generator=gen)[:60]
    nz[:3] = torch.tensor([g.U, g.U + 1, 5])                               # the hot items and an isolated user among the flagged rows
    Gs = torch.zeros(g.N, d)
    Gs[nz] = torch.randn(60, d, generator=gen)
    flags = torch.zeros(g.N, dtype=torch.uint8); flags[nz] = 1
    return Gs.to(DEV), flags.to(DEV), nz.to(torch.int32).to(DEV)


@case('spmm_flagged')
def _(ops):
    g, gb = graph(ops), graph(ops, True)
    ins = {d: flag_inputs(g, d, 40 + d) for d in WIDTHS}
    X64 = spmm_inputs(g, 64, 41)[0]

    def run(caller):
        r = {}
        for d, (Gs, flags, nz) in ins.items():
            bits = torch.zeros((g.N + 31) // 32, dtype=torch.int32, device=DEV)
            ops.mark_bits_(bits, nz, True, g.N)
            r['masked%d' % d] = ops.spmm_flagged(g.A, Gs, bits, 1.0, 1.0, Gs, flags, out=Pz(g.N, d) if caller else None)
        Gs, flags, _ = ins[64]
        r['dense64'] = ops.spmm_flagged(g.A, X64, None, 0.5, 2.0, Gs, flags, out=Pz(g.N, 64) if caller else None)
        r['blocked64'] = ops.spmm_flagged(gb.A, X64, None, 0.5, 2.0, Gs, flags, out=Pz(g.N, 64) if caller else None)
        return r

    def ref():
        r = {'masked%d' % d: g.M @ Gs.double() + Gs.double() for d, (Gs, _, _) in ins.items()}
        r['dense64'] = r['blocked64'] = 0.5 * (g.M @ X64.double()) + 2.0 * ins[64][0].double()
        return r
    return run, ref


@case('spmm_rows')
def _(ops):
    g = graph(ops)
    rng = np.random.default_rng(50)
    rows = T(np.concatenate([rng.integers(0, g.N, 70), [g.U, g.U, g.U + 1, 5, 77, 0]]).astype(np.int32))       # 76 rows: hot, empty, duplicates
    ins = {d: spmm_inputs(g, d, 50 + d) for d in WIDTHS}
    rw = torch.rand(rows.numel(), generator=torch.Generator().manual_seed(51)).to(DEV)

    def run(caller):
        r = {}
        for d, (X, L1, _, _) in ins.items():
            for ns in (1, 5):
                need = ops._lib.lib().arl_spmm_csr_rows_workspace_bytes(rows.numel(), ns, d) // 4
                kw = dict(out=Pz(rows.numel(), d), workspace=Pz(need + 3)) if caller else {}
                r['d%d_ns%d' % (d, ns)] = ops.spmm_rows(g.A, X, rows, [X, L1], 0.25, nsplit=ns, row_weight=rw if ns == 5 else None, **kw)
        return r

    def ref():
        r = {}
        for d, (X, L1, _, _) in ins.items():
            full = (X.double() + L1.double())[rows.long()]
            prod = (g.M @ X.double())[rows.long()]
            r['d%d_ns1' % d] = 0.25 * (full + prod)
            r['d%d_ns5' % d] = 0.25 * rw.double()[:, None] * (full + prod)         # row_weight scales the whole listed row
        return r
    return run, ref


def loss_problem(d, seed, B=67, U=300, I=200):
    from test_gpu_width_classes import loss_batch
    rng = np.random.default_rng(seed)
    E = (rng.standard_normal((U + I, d)) * (0.6 / np.sqrt(d))).astype(np.float32)
    return E, U, loss_batch(B, U, I, seed + 1)


def _loss_case(ops, which):
    from test_gpu_width_classes import bpr64, wrmf64
    probs = {d: loss_problem(d, 60 + d) for d in WIDTHS}

    def run(caller):
        r = {}
        for d, (E, U, (u, p, n)) in probs.items():
            G = torch.zeros(E.shape[0], d, device=DEV)
            B = len(u)
            if which == 'bpr':
                kw = dict(workspace=Pz(4 * B), loss_out=Pz(4)) if caller else {}
                lo = ops.bpr_l2_fwd_bwd(T(E), U, T(u), T(p), T(n), 1e-2, G, upstream=0.5, **kw)
            else:
                kw = dict(workspace=Pz(5 * B), loss_out=Pz(4)) if caller else {}
                lo = ops.wrmf_l2_fwd_bwd(T(E), U, T(u), T(p), T(n), 1e-2, 20.0, G, upstream=0.5, **kw)
            r['loss%d' % d], r['G%d' % d] = lo, G
        return r

    def ref():
        r = {}
        for d, (E, U, (u, p, n)) in probs.items():
            lo, gr = (bpr64(E, U, u, p, n, 1e-2, upstream=0.5) if which == 'bpr' else wrmf64(E, U, u, p, n, 1e-2, 20.0, upstream=0.5))
            r['loss%d' % d], r['G%d' % d] = torch.from_numpy(lo), torch.from_numpy(gr)
        return r
    return run, ref


@case('bpr_l2_fwd_bwd')
def _(ops):
    return _loss_case(ops, 'bpr')


@case('wrmf_l2_fwd_bwd')
def _(ops):
    return _loss_case(ops, 'wrmf')


def _bpr_pair(ops):
    """bpr_l2_partial on two ragged halves + the caller's reduction + bpr_l2_backward of each half (the sharded pair)."""
    from test_gpu_width_classes import bpr64
    probs = {d: loss_problem(d, 70 + d) for d in (12, 100)}

    def run(caller):
        r = {}
        for d, (E, U, (u, p, n)) in probs.items():
            B, h, reg = len(u), len(u) // 2 + 1, 1e-2
            parts = [(T(u[a:b]), T(p[a:b]), T(n[a:b])) for a, b in ((0, h), (h, B))]
            wss = [(Pz if caller else (lambda k: torch.empty(k, device=DEV)))(4 * b.numel()) for b, _, _ in parts]
            sums = torch.zeros(3, device=DEV)
            for (bu, bp, bn), ws in zip(parts, wss):
                sums = sums + ops.bpr_l2_partial(T(E), U, bu, bp, bn, B, ws, Pz(3) if caller else torch.empty(3, device=DEV))
            nu, npn = torch.sqrt(sums[1]), torch.sqrt(sums[2])
            norms4 = torch.stack([sums[0] / B, reg * (nu + npn), nu, npn]).contiguous()
            G = torch.zeros(E.shape[0], d, device=DEV)
            for (bu, bp, bn), ws in zip(parts, wss):
                ops.bpr_l2_backward(T(E), U, bu, bp, bn, reg, norms4, G, ws)
            r['norms%d' % d], r['G%d' % d] = norms4, G
        return r

    def ref():
        r = {}
        for d, (E, U, (u, p, n)) in probs.items():
            lo, gr = bpr64(E, U, u, p, n, 1e-2)
            r['norms%d' % d], r['G%d' % d] = torch.from_numpy(lo), torch.from_numpy(gr)
        return r
    return run, ref


CASES['bpr_l2_partial'] = CASES['bpr_l2_backward'] = _bpr_pair


@case('gather_rows')
def _(ops):
    gen = torch.Generator().manual_seed(80)
    srcs = {d: randn(gen, 131, d) for d in WIDTHS + (3,)}
    idx = torch.randint(0, 131, (77,), generator=gen).to(torch.int32).to(DEV)
    return (lambda caller: {'d%d' % d: ops.gather_rows(s, idx) for d, s in srcs.items()},
            lambda: {'d%d' % d: s.double()[idx.long()] for d, s in srcs.items()})


@case('shard_batch_prep')
def _(ops):
    gen = torch.Generator().manual_seed(81)
    B, u0, u1 = 67, 40, 170
    u, p, n = (torch.randint(0, hi, (B,), generator=gen).to(torch.int32).to(DEV) for hi in (300, 200, 200))

    def run(caller):
        out = (Pz(B, dtype=torch.int32), Pz(3 * B), Pz(2 * B, dtype=torch.int32), Pz(3 * B, dtype=torch.int32)) if caller else None
        return dict(zip(('lu', 'own', 'item_rows', 'rows_l'), ops.shard_batch_prep(u, p, n, u0, u1, out=out)))

    def ref():
        mine = (u >= u0) & (u < u1)
        Ul = u1 - u0
        lu = (u - u0).clamp(0, Ul - 1)
        return {'own': (torch.cat([mine.double(), torch.ones(2 * B, dtype=torch.float64, device=DEV)]), 0.0), 'item_rows': (torch.cat([p, n]).double(), 0.0),
                'lu': (lu.double(), 0.0), 'rows_l': (torch.cat([lu, Ul + p, Ul + n]).double(), 0.0)}
    return run, ref


@case('infonce_fwd_bwd')
def _(ops):
    from test_gpu_width_classes import infonce64
    rng = np.random.default_rng(82)
    ins = {}
    for d in WIDTHS:
        v1 = rng.standard_normal((65, d)).astype(np.float32)
        ins[d] = (v1, (v1 + 0.5 * rng.standard_normal((65, d))).astype(np.float32))

    def run(caller):
        r = {}
        for d, (v1, v2) in ins.items():
            r['loss%d' % d], r['d1_%d' % d], r['d2_%d' % d] = ops.infonce_fwd_bwd(T(v1), T(v2), 0.2, upstream=0.7)
        return r

    def ref():
        r = {}
        for d, (v1, v2) in ins.items():
            l, a, b = infonce64(v1, v2, 0.2, 0.7)
            r['loss%d' % d], r['d1_%d' % d], r['d2_%d' % d] = torch.tensor([l], dtype=torch.float64), torch.from_numpy(a), torch.from_numpy(b)
        return r
    return run, ref


@case('nce_allrows')
def _(ops):
    gen = torch.Generator().manual_seed(83)
    nrm = lambda t: torch.nn.functional.normalize(t, dim=1)
    ins = {d: (nrm(randn(gen, 77, d)), nrm(randn(gen, 333, d))) for d in MFMA_WIDTHS}
    ins[32] = (nrm(randn(gen, 70, 32)), nrm(randn(gen, 9001, 32)))        # more than one split of the streamed table: partial tiles folded
    tau = 0.2

    def run(caller):
        r = {}
        for d, (A, V) in ins.items():
            lse0 = ops.nce_allrows(A, V, tau, want_grad=False)
            lse, dA, dV = ops.nce_allrows(A, V, tau)
            lse2, dA2, _ = ops.nce_allrows(A, V, tau, want_dV=False, lse=lse0.clone())
            r.update({'lse0_%d' % d: lse0, 'lse_%d' % d: lse, 'dA_%d' % d: dA, 'dV_%d' % d: dV, 'dA2_%d' % d: dA2})
        return r

    def ref():
        r = {}
        for d, (A, V) in ins.items():
            lg = A.double() @ V.double().T / tau
            lse = torch.logsumexp(lg, 1)
            Pm = torch.exp(lg - lse[:, None])
            r.update({'lse0_%d' % d: (lse, RTOL), 'lse_%d' % d: (lse, RTOL), 'dA_%d' % d: (Pm @ V.double(), RTOL), 'dV_%d' % d: (Pm.T @ A.double(), RTOL),
                      'dA2_%d' % d: (Pm @ V.double(), RTOL)})
        return r
    return run, ref


@case('ssl_dropout_nce')
def _(ops):
    from test_gpu_ssl4rec import ref_term, rand_rows, rand_masks
    ins = {d: rand_rows(37 if d == 16 else 300, d, 84 + d) + (rand_masks(37 if d == 16 else 300, d, 85 + d),) for d in MFMA_WIDTHS}

    def run(caller):
        r = {}
        for d, (Xu, Xp, masks) in ins.items():
            loss, (Gu, Gp) = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, masks=masks)
            loss2, (Gu2, _) = ops.ssl_dropout_nce(Xu, Xp, 0.2, 0.2, seed=5, stream_id=d)
            r.update({'loss%d' % d: loss, 'Gu%d' % d: Gu, 'Gp%d' % d: Gp, 'drawn_loss%d' % d: loss2, 'drawn_Gu%d' % d: Gu2})
        return r

    def ref():
        r = {}
        for d, (Xu, Xp, masks) in ins.items():
            lu, lp, gu, gp = ref_term(Xu, Xp, masks)
            r.update({'loss%d' % d: (torch.tensor([lu, lp], dtype=torch.float64), TOL), 'Gu%d' % d: (gu, RTOL, True), 'Gp%d' % d: (gp, RTOL, True)})
        return r
    return run, ref


@case('normalize_rows')
def _(ops):
    gen = torch.Generator().manual_seed(86)
    ins = {d: randn(gen, 65, d) for d in WIDTHS}

    def run(caller):
        r = {}
        for d, X in ins.items():
            r['Y%d' % d], r['nrm%d' % d] = ops.normalize_rows(X)
        return r

    def ref():
        r = {}
        for d, X in ins.items():
            nr = X.double().norm(dim=1).clamp_min(1e-12)
            r['Y%d' % d], r['nrm%d' % d] = X.double() / nr[:, None], nr
        return r
    return run, ref


@case('normalize_rows_bwd')
def _(ops):
    gen = torch.Generator().manual_seed(87)
    ins = {d: (randn(gen, 65, d), randn(gen, 65, d)) for d in WIDTHS}

    def run(caller):
        r = {}
        for d, (X, dY) in ins.items():
            Y, nrm = ops.normalize_rows(X)
            r['dX%d' % d] = ops.normalize_rows_bwd(Y, nrm, dY, 0.5, out=Pz(65, d) if caller else None)
        return r

    def ref():
        r = {}
        for d, (X, dY) in ins.items():
            nr = X.double().norm(dim=1, keepdim=True)
            Y = X.double() / nr
            r['dX%d' % d] = 0.5 * (dY.double() - Y * (Y * dY.double()).sum(1, keepdim=True)) / nr
        return r
    return run, ref


@case('simgcl_perturb_rng')
def _(ops):
    gen = torch.Generator().manual_seed(88)
    ins = {d: randn(gen, 65, d) for d in WIDTHS + (3,)}

    def run(caller):
        r = {}
        for d, X in ins.items():
            out = ops.simgcl_perturb_rng(X, 0.1, 7, 3, out=Pz(65, d) if caller else None)
            r['d%d' % d], r['len%d' % d], r['sign%d' % d] = out, (out - X).norm(dim=1), ((out - X) * X >= 0).float().mean().view(1)
        return r

    def ref():           # the perturbation has length eps per row and the sign of the source (the draw itself is pinned by test_simgcl_perturb_rng)
        r = {}
        for d in ins:
            r['len%d' % d], r['sign%d' % d] = (torch.full((65,), 0.1, dtype=torch.float64), RTOL), (torch.ones(1, dtype=torch.float64), 0.0)
        return r
    return run, ref


@case('sfa_l1')
def _(ops):
    gen = torch.Generator().manual_seed(89)
    ins = {}
    for d in WIDTHS + (3,):
        n = 777 if d == 64 else 67
        w = torch.randint(0, 4, (n,), generator=gen).float()
        w[0] = 3.0
        ins[d] = (randn(gen, n, d), w.to(DEV), randn(gen, d), int(w.sum().item()) * d)

    def run(caller):
        r = {}
        for d, (X, w, r0, numel) in ins.items():
            r['loss%d' % d], r['G%d' % d] = ops.sfa_l1(X, w, r0, numel, out=Pz(*X.shape) if caller else None, scale=0.5)
            r['loss_only%d' % d] = ops.sfa_l1(X, w, r0, numel, want_grad=False)[0]
        return r

    def ref():
        from oracle import oracle as O                                    # the literal restatement on H, as test_sfa_l1_weighted_rows
        r = {}
        for d, (X, w, r0, numel) in ins.items():
            rows = np.repeat(np.arange(X.shape[0]), w.cpu().numpy().astype(np.int64))
            loss_ref, gH = O.sfa_l1_loss_grad(X.cpu().numpy()[rows], r0.cpu().numpy())
            G_ref = np.zeros(tuple(X.shape)); np.add.at(G_ref, rows, gH)
            r['loss%d' % d] = r['loss_only%d' % d] = (torch.tensor([loss_ref], dtype=torch.float64), RTOL)
            r['G%d' % d] = (torch.from_numpy(0.5 * G_ref), RTOL)
        return r
    return run, ref


@case('SfaStages')
def _(ops):
    gen = torch.Generator().manual_seed(90)
    X, w, r0 = randn(gen, 777, 100), torch.randint(0, 4, (777,), generator=gen).float().to(DEV), randn(gen, 100)
    numel = int(w.sum().item()) * 100

    def run(caller):
        st = ops.SfaStages(X, w, r0)
        if caller:
            poison_(st.ws)
        r = st.stage1()
        a_s = st.stage2(r)
        loss, G = st.stage3(r, a_s, numel, out=Pz(*X.shape) if caller else None, scale=0.5)
        return {'r': r, 'a_s': a_s, 'loss': loss, 'G': G}

    def ref():           # the one-call form is the float64-checked one (test_sfa_l1_weighted_rows); the stages must reproduce it
        loss, G = ops.sfa_l1(X, w, r0, numel, scale=0.5)
        return {'loss': (loss.double(), TOL), 'G': (G.double(), TOL)}
    return run, ref


@case('sddmm_rows_dense')
def _(ops):
    gen = torch.Generator().manual_seed(91)
    ins = {d: (randn(gen, 40, d), randn(gen, 131, d)) for d in WIDTHS + (3,)}
    rows = torch.tensor([0, 39, 7, 7, 12], dtype=torch.int32, device=DEV)

    def run(caller):
        r = {}
        for d, (dY, X) in ins.items():
            out = torch.zeros(5, 83, device=DEV)
            r['d%d' % d] = ops.sddmm_rows_dense(dY, X, rows, 48, 83, out=out)
            r['alloc%d' % d] = ops.sddmm_rows_dense(dY, X, rows, 48, 83)
        return r

    def ref():
        r = {}
        for d, (dY, X) in ins.items():
            r['d%d' % d] = r['alloc%d' % d] = dY.double()[rows.long()] @ X.double()[48:131].T
        return r
    return run, ref


@case('sddmm_csr')
def _(ops):
    g = graph(ops)
    gen = torch.Generator().manual_seed(92)
    ins = {d: (randn(gen, g.N, d), randn(gen, g.N, d)) for d in WIDTHS}
    col = T(g.col).long()

    def run(caller):
        return {'d%d' % d: ops.sddmm_csr(g.A, dY, X, 0.5) for d, (dY, X) in ins.items()}

    def ref():
        return {'d%d' % d: 0.5 * (dY.double()[g.erow.long()] * X.double()[col]).sum(1) for d, (dY, X) in ins.items()}
    return run, ref


@case('tables_sum')
def _(ops):
    gen = torch.Generator().manual_seed(93)
    tabs = [randn(gen, 67, 12) for _ in range(5)]
    return (lambda caller: {'sum': ops.tables_sum(tabs, 0.2, out=Pz(67, 12) if caller else None), 'one': ops.tables_sum(tabs[:1], 1.0)},
            lambda: {'sum': 0.2 * sum(t.double() for t in tabs), 'one': tabs[0].double()})


def fb_inputs(F, I, d, seed):
    gen = torch.Generator().manual_seed(seed)
    S = (torch.rand(F, I, generator=gen) * (torch.rand(F, I, generator=gen) < 0.3)).to(DEV)
    return S, randn(gen, I, d), randn(gen, F, d), randn(gen, I, d), randn(gen, F, d), torch.rand(F, generator=gen).to(DEV), torch.rand(I, generator=gen).to(DEV)


@case('fake_block_rows_')
def _(ops):
    shapes = [(5, 777, 12), (130, 301, 64), (7, 1345, 100), (1, 4, 256)]
    ins = [fb_inputs(F, I, d, 94 + F) for F, I, d in shapes]

    def run(caller):
        r = {}
        for k, (S, X, Y, _, _, rs, _) in enumerate(ins):
            if caller:       # the op's caller-visible buffer is its cached workspace (keyed by size): a first call of this problem leaves it, then it is poisoned
                ops.fake_block_rows_(S, X, Y.clone(), rs, 0.5)
                assert len(ops._FB_WS) == 1
                for ws in ops._FB_WS.values():
                    poison_(ws)
            r['Y%d' % k] = ops.fake_block_rows_(S, X, Y.clone(), rs, 0.5)
        return r
    return run, lambda: {'Y%d' % k: Y.double() + 0.5 * rs.double()[:, None] * (S.double() @ X.double()) for k, (S, X, Y, _, _, rs, _) in enumerate(ins)}


@case('fake_block_cols_')
def _(ops):
    shapes = [(5, 777, 12), (130, 301, 64), (7, 1345, 100), (1, 4, 256)]
    ins = [fb_inputs(F, I, d, 95 + F) for F, I, d in shapes]
    # (no workspace and no out=: `caller` has nothing to poison, the run is listed for the in-place operand under poisoned allocations)
    return (lambda caller: {'Y%d' % k: ops.fake_block_cols_(S, Xf, Yi.clone(), cs, 0.5) for k, (S, _, _, Yi, Xf, _, cs) in enumerate(ins)},
            lambda: {'Y%d' % k: Yi.double() + 0.5 * cs.double()[:, None] * (S.double().T @ Xf.double()) for k, (S, _, _, Yi, Xf, _, cs) in enumerate(ins)})


def cw_problem(Up, F, I, d, k, nT, seed):
    gen = torch.Generator().manual_seed(seed)
    X = randn(gen, Up + I, d, scale=0.1)
    top = torch.stack([torch.randperm(I, generator=gen)[:k] for _ in range(Up)]).to(torch.int32)
    top[: Up // 2, k - 1] = 3                                              # a popular negative: long bucket, duplicates across users
    targets = torch.randperm(I, generator=gen)[:nT]
    return X, Up, Up - F, top.to(DEV), targets.to(DEV)


CW_SHAPES = [(257, 1, 300, 100, 64, 64), (500, 0, 70, 12, 8, 3), (130, 3, 1000, 64, 20, 5), (67, 2, 150, 256, 10, 1)]


@case('cw_topk_term')
def _(ops):
    from test_gpu_attack_edges import cw_ref64
    probs = [cw_problem(*s, seed=96 + k) for k, s in enumerate(CW_SHAPES)]

    def run(caller):
        r = {}
        for k, (X, Up, n_real, top, tg) in enumerate(probs):
            if caller:       # as fake_block_rows_: the cached workspace of THIS problem's size, left by a first call, poisoned before the call that counts
                ops.cw_topk_term(X, Up, n_real, top, tg)
                assert len(ops._CW_WS) == 1
                for ws in ops._CW_WS.values():
                    poison_(ws)
            r['loss%d' % k], r['G%d' % k], r['w%d' % k] = ops.cw_topk_term(X, Up, n_real, top, tg)
        return r

    def ref():
        r = {}
        for k, (X, Up, n_real, top, tg) in enumerate(probs):
            loss, G, w, mag = cw_ref64(X, Up, n_real, top, tg)
            r['G%d' % k], r['w%d' % k] = (G, RTOL, True), (w, 0.0)
            r['loss%d' % k] = (loss.view(1), TOL * max(mag / max(abs(loss.item()), 1e-300), 1.0))
        return r
    return run, ref


def topk_problem(U, I, d, masked, seed):
    gen = torch.Generator().manual_seed(seed)
    Pu, Pi = randn(gen, U, d), randn(gen, I, d)
    rp = mc = None
    if masked:
        cnt = torch.randint(0, 9, (U,), generator=gen)
        cnt[0] = 0
        rp = torch.zeros(U + 1, dtype=torch.int64); rp[1:] = torch.cumsum(cnt, 0)
        mc = torch.cat([torch.sort(torch.randperm(I, generator=gen)[:c])[0] for c in cnt.tolist()] + [torch.zeros(0, dtype=torch.int64)])
        rp, mc = rp.to(torch.int32).to(DEV), (mc if mc.numel() else torch.zeros(1, dtype=torch.int64)).to(torch.int32).to(DEV)
    return Pu, Pi, rp, mc


TOPK_SHAPES = [(37, 301, 64, 50, True, False), (37, 301, 64, 50, True, True), (70, 515, 32, 128, True, False), (33, 301, 12, 5, False, False),
               (17, 301, 128, 20, False, False), (100, 1412, 64, 7, False, False)]


@case('score_mask_topk')
def _(ops):
    probs = [topk_problem(U, I, d, m, 97 + k) for k, (U, I, d, _, m, _) in enumerate(TOPK_SHAPES)]

    def run(caller):
        r = {}
        for k, ((Pu, Pi, rp, mc), (_, _, _, kk, _, exact)) in enumerate(zip(probs, TOPK_SHAPES)):
            ops.reset_exit_probe()
            r['idx%d' % k], r['val%d' % k] = ops.score_mask_topk(Pu, Pi, kk, rp, mc, exact=exact)
            if not exact and Pu.shape[1] == 64:
                r['warm_idx%d' % k], r['warm_val%d' % k] = ops.score_mask_topk(Pu, Pi, kk, rp, mc, warm_idx=r['idx%d' % k].clone())
            if not exact and Pu.shape[1] in (64, 128):      # a caller's item order: the inverse map and the two builds' gate words are in use
                order = torch.randperm(Pi.shape[0], generator=torch.Generator().manual_seed(k)).to(torch.int32).to(DEV)
                r['ord_idx%d' % k], r['ord_val%d' % k] = ops.score_mask_topk(Pu, Pi, kk, rp, mc, item_order=order)
                assert ops._EXIT_PROBE
        return r

    def ref():
        r = {}
        for k, ((Pu, Pi, rp, mc), (U, I, _, kk, _, _)) in enumerate(zip(probs, TOPK_SHAPES)):
            sc = Pu.double() @ Pi.double().T
            if rp is not None:
                rows = torch.repeat_interleave(torch.arange(U, device=DEV), (rp[1:] - rp[:-1]).long())
                sc[rows, mc.long()[:rows.numel()]] = -10e8
            r['val%d' % k] = (torch.topk(sc, kk, dim=1)[0], RTOL)
            if Pu.shape[1] in (64, 128) and not TOPK_SHAPES[k][5]:
                r['ord_val%d' % k] = r['val%d' % k]
        return r
    return run, ref


@case('topn_project_rows')
def _(ops):
    gen = torch.Generator().manual_seed(98)
    M = torch.rand(7, 301, generator=gen).to(DEV)

    def run(caller):
        out, idx = ops.topn_project_rows(M, 10)
        return {'out': out, 'idx': idx}

    def ref():
        from oracle import oracle as O
        ro, ri = O.topn_project_rows(M.cpu().numpy(), 10)
        return {'out': (torch.from_numpy(ro.astype(np.float64)), 0.0), 'idx': (torch.from_numpy(ri.astype(np.float64)), 0.0)}
    return run, ref


def _ngcf_inputs(seed, n_of=lambda d: 67):
    gen = torch.Generator().manual_seed(seed)
    return {d: (randn(gen, n_of(d), d), randn(gen, n_of(d), d), randn(gen, n_of(d), 2 * d)) for d in (12, 64, 100)}


@case('ngcf_combine')
def _(ops):
    ins = _ngcf_inputs(99)
    return (lambda caller: {'d%d' % d: ops.ngcf_combine(P, E, out=Pz(67, 2 * d) if caller else None) for d, (P, E, _) in ins.items()},
            lambda: {'d%d' % d: torch.cat([P.double() + E.double(), P.double() * E.double()], 1) for d, (P, E, _) in ins.items()})


@case('ngcf_combine_bwd')
def _(ops):
    ins = _ngcf_inputs(100)

    def run(caller):
        r = {}
        for d, (P, E, g) in ins.items():
            r['gP%d' % d], r['gE%d' % d] = ops.ngcf_combine_bwd(g, P, E)
        return r

    def ref():
        r = {}
        for d, (P, E, g) in ins.items():
            gs, gt = g.double()[:, :d], g.double()[:, d:]
            r['gP%d' % d], r['gE%d' % d] = gs + gt * E.double(), gs + gt * P.double()
        return r
    return run, ref


@case('ngcf_act_bwd')
def _(ops):
    ins = _ngcf_inputs(101)
    return (lambda caller: {'d%d' % d: ops.ngcf_act_bwd(P, E, 0.01) for d, (P, E, _) in ins.items()},
            lambda: {'d%d' % d: P.double() * torch.where(E > 0, 1.0, 0.01).double() for d, (P, E, _) in ins.items()})


def dense_inputs(seed):
    gen = torch.Generator().manual_seed(seed)
    r = {}
    for d, n in ((16, 67), (64, 1000), (32, 0)):                          # n = 0: the weight-gradient entry's special case
        r[(d, n)] = (randn(gen, n, d, scale=0.5), randn(gen, n, d, scale=0.5), randn(gen, 2 * d, d, scale=0.3), randn(gen, n, d))
    return r


def dense64(P, E, W, slope=0.01):
    ST = torch.cat([P.double() + E.double(), P.double() * E.double()], 1)
    Z = ST @ W.double()
    return torch.where(Z > 0, Z, slope * Z), ST, Z


@case('ngcf_dense_fwd')
def _(ops):
    ins = {k: v for k, v in dense_inputs(102).items() if k[1] > 0}
    return (lambda caller: {'d%d' % d: ops.ngcf_dense_fwd(P, E, W, out=Pz(n, d) if caller else None) for (d, n), (P, E, W, _) in ins.items()},
            lambda: {'d%d' % d: (dense64(P, E, W)[0], RTOL) for (d, n), (P, E, W, _) in ins.items()})


@case('ngcf_dense_bwd')
def _(ops):
    ins = dense_inputs(103)

    def run(caller):
        r = {}
        for (d, n), (P, E, W, gO) in ins.items():
            if n == 0:       # the entry's own n = 0 case (gW memset), through the C ABI: an empty tensor's pointer is NULL, which the entry refuses first
                one, gW = torch.zeros(1, d, device=DEV), (Pz(2 * d, d) if caller else torch.empty(2 * d, d, device=DEV))
                ops.check(ops._lib.lib().arl_ngcf_dense_wgrad_f32(ops._ptr(one), ops._ptr(one), ops._ptr(one), 0, d, ops._ptr(gW), ops._ptr(torch.empty(4, device=DEV)),
                                                                  ops._stream()), 'arl_ngcf_dense_wgrad_f32')
                r['gW%d' % d] = gW
                continue
            out = ops.ngcf_dense_fwd(P, E, W)
            r['gP%d' % d], r['gE%d' % d], r['gW%d' % d] = ops.ngcf_dense_bwd(gO, out, P, E, W)
        return r

    def ref():
        r = {}
        for (d, n), (P, E, W, gO) in ins.items():
            if n == 0:
                r['gW%d' % d] = (torch.zeros(2 * d, d, dtype=torch.float64, device=DEV), 0.0)
                continue
            out = ops.ngcf_dense_fwd(P, E, W)
            _, ST, _ = dense64(P, E, W)
            gZ = gO.double() * torch.where(out > 0, 1.0, 0.01).double()      # the kernel's own side of the kink (its forward output)
            gST = gZ @ W.double().T
            r['gW%d' % d] = (ST.T @ gZ, RTOL)
            r['gP%d' % d] = (gST[:, :d] + gST[:, d:] * E.double(), RTOL)
            r['gE%d' % d] = (gST[:, :d] + gST[:, d:] * P.double(), RTOL)
        return r
    return run, ref


def tower_inputs(seed):
    from test_gpu_ncf import weights, f32
    r = {}
    for d, n in ((16, 17), (64, 301), (32, 0)):
        gen = torch.Generator().manual_seed(seed + d)
        N = 131
        mf, mlp = torch.randn(N, d, generator=gen, dtype=torch.float64), torch.randn(N, d, generator=gen, dtype=torch.float64)
        W = weights(d, gen)
        rows = torch.randint(0, N, (n,), generator=gen)
        if n:
            rows[: n // 3] = rows[0]
        r[(d, n)] = (mf, mlp, W, rows, torch.randn(n, 2 * d, generator=gen, dtype=torch.float64), f32((mf, mlp)), f32(W), rows.to(torch.int32).to(DEV))
    return r


@case('ncf_tower_fwd')
def _(ops):
    from test_gpu_ncf import ref_tower
    ins = {k: v for k, v in tower_inputs(104).items() if k[1] > 0}

    def run(caller):
        r = {}
        for (d, n), (_, _, _, _, _, (mf_d, mlp_d), Wd, rows_d) in ins.items():
            r['out%d' % d], r['h1_%d' % d], r['h2_%d' % d] = ops.ncf_tower_fwd(mf_d, mlp_d, Wd, rows_d)
            r['table%d' % d] = ops.ncf_tower_fwd(mf_d, mlp_d, Wd)
        return r

    def ref():
        r = {}
        for (d, n), (mf, mlp, W, rows, _, _, _, _) in ins.items():
            r['out%d' % d] = (ref_tower(mf, mlp, W, rows), RTOL, True)
            r['table%d' % d] = (ref_tower(mf, mlp, W, torch.arange(mf.shape[0])), RTOL, True)
        return r
    return run, ref


@case('ncf_tower_bwd')
def _(ops):
    ins = tower_inputs(105)

    def run(caller):
        r = {}
        for (d, n), (_, _, _, _, gout, (mf_d, mlp_d), Wd, rows_d) in ins.items():
            if n == 0:       # the entry's own n = 0 case (parameter gradients memset), through the C ABI with one-row stand-ins for the empty operands
                z = lambda w: torch.zeros(1, w * d, device=DEV)
                flat = Pz(17 * d * d + 8 * d) if caller else torch.empty(17 * d * d + 8 * d, device=DEV)
                p_ = ops._ptr
                ops.check(ops._lib.lib().arl_ncf_tower_bwd_f32(p_(z(2)), p_(z(2)), p_(z(5)), p_(z(2)), p_(mlp_d), None, 0, d, p_(Wd[0]), p_(Wd[2]), p_(Wd[4]), p_(z(1)),
                                                               p_(flat), p_(torch.empty(4, device=DEV)), ops._stream()), 'arl_ncf_tower_bwd_f32')
                off = 0
                for j, w in enumerate(Wd):
                    r['gW%d_%d' % (j, d)] = flat[off:off + w.numel()].view(w.shape)
                    off += w.numel()
                continue
            out, h1, h2 = ops.ncf_tower_fwd(mf_d, mlp_d, Wd, rows_d)
            g_rows, gW = ops.ncf_tower_bwd(gout.float().to(DEV), out, h1, h2, mlp_d, Wd, rows_d)
            r['g_rows%d' % d] = g_rows
            for j, t in enumerate(gW):
                r['gW%d_%d' % (j, d)] = t
        return r

    def ref():
        r = {}
        for (d, n), (mf, mlp, W, rows, gout, _, _, _) in ins.items():
            if n == 0:
                for j, w in enumerate(W):
                    r['gW%d_%d' % (j, d)] = (torch.zeros_like(w), 0.0)
                continue
            x = mlp[rows].clone().requires_grad_(True)
            Wr = [w.clone().requires_grad_(True) for w in W]
            h = x
            for k in range(3):
                h = torch.relu(h @ Wr[2 * k].T + Wr[2 * k + 1])
            (h * gout[:, d:]).sum().backward()
            r['g_rows%d' % d] = (x.grad, RTOL, True)
            for j, w in enumerate(Wr):
                r['gW%d_%d' % (j, d)] = (w.grad, RTOL, w.dim() == 2)
        return r
    return run, ref


# GAN ops: M, N, K straddling the 128 x 128 x 16 tile of the gemm, F and S ragged against the 64-row / 256-column blocks of the row kernels
@case('gan_gemm')
def _(ops):
    gen = torch.Generator().manual_seed(107)
    A, B = randn(gen, 131, 77), randn(gen, 77, 259)
    A2, B2 = randn(gen, 127, 15), randn(gen, 15, 129)
    bias, aux, bias2, aux2 = randn(gen, 259), randn(gen, 131, 259), randn(gen, 129), randn(gen, 127, 129)
    combos = [(ta, tb) for ta in (False, True) for tb in (False, True)]

    def run(caller):
        r = {}
        for tag, (a0, b0, bi, au) in (('a', (A, B, bias, aux)), ('b', (A2, B2, bias2, aux2))):
            for ta, tb in combos:
                a = a0.t().contiguous() if ta else a0
                b = b0.t().contiguous() if tb else b0
                for epi in (ops.GAN_EPI_STORE, ops.GAN_EPI_BIAS_SIGMOID, ops.GAN_EPI_RELU_MASK):
                    r['%s%d%d_%d' % (tag, ta, tb, epi)] = ops.gan_gemm(a, b, ta, tb, epi, bias=bi, aux=au)
        return r

    def ref():
        r = {}
        for tag, (a0, b0, bi, au) in (('a', (A, B, bias, aux)), ('b', (A2, B2, bias2, aux2))):
            Cm = a0.double() @ b0.double()
            outs = (Cm, torch.sigmoid(Cm + bi.double()), torch.where(au > 0, Cm, torch.zeros_like(Cm)))
            for ta, tb in combos:
                for epi in range(3):
                    r['%s%d%d_%d' % (tag, ta, tb, epi)] = (outs[epi], 1e-6 if epi == 0 else TOL)
        return r
    return run, ref


def gan_problem():
    from test_gpu_aush import make_problem
    return make_problem(37, 1003, 5, seed=108, empty_rows=(0, 36))


@case('gan_spmm')
def _(ops):
    tpl, P = gan_problem()
    W1t = P[0].t().contiguous()

    def run(caller):
        return {'relu': ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, W1t, bias=P[1], relu=True), 'plain': ops.gan_spmm(tpl.rowptr, tpl.col, tpl.val, W1t)}

    def ref():
        Z = tpl.Td.double() @ W1t.double()
        return {'relu': (torch.relu(Z + P[1].double()), TOL), 'plain': (Z, TOL)}
    return run, ref


@case('gan_transpose')
def _(ops):
    A = randn(torch.Generator().manual_seed(109), 37, 1003)
    return (lambda caller: {'t': ops.gan_transpose(A), 't2': ops.gan_transpose(A[:33, :31].contiguous())},
            lambda: {'t': (A.double().t(), 0.0), 't2': (A[:33, :31].double().t(), 0.0)})


def gan_rows_inputs():
    tpl, P = gan_problem()
    gen = torch.Generator().manual_seed(110)
    Y = torch.rand(37, 1003, generator=gen).to(DEV)
    return tpl, Y, P[4].reshape(-1).contiguous(), P[5], 5


@case('gan_rows')
def _(ops):
    tpl, Y, wD, bD, Tn = gan_rows_inputs()
    Td = tpl.Td

    def run(caller):
        return dict(zip(('rows', 'losses', 'coef', 'pf'), ops.gan_rows(Y, Td, Tn, wD, bD)))

    def ref():
        Yd, Tdd, w = Y.double(), Td.double(), wD.double()
        rows = torch.stack([Yd @ w, Tdd @ w, ((Yd - Tdd) ** 2).sum(1), (1 - Yd[:, -Tn:]).sum(1)], 1)
        return {'rows': (rows, TOL), 'pf': (torch.sigmoid(rows[:, 0] + bD.double()), TOL)}       # sums of 1003 fp32 terms: ~2e-6
    return run, ref


@case('gan_dz2')
def _(ops):
    tpl, Y, wD, bD, Tn = gan_rows_inputs()
    Td = tpl.Td

    def run(caller):
        rows, losses, coef, pf = ops.gan_rows(Y, Td, Tn, wD, bD)
        return {'dZ2': ops.gan_dz2(Y, Td, rows, pf, wD, Tn)}

    def ref():
        Yr = Y.double().requires_grad_(True)
        Df = torch.sigmoid(Yr @ wD.double() + bD.double())
        loss2 = torch.log(1 - Df).mean() + ((1 - Yr[:, -Tn:]).sum(1) ** 2).mean() + ((Yr - Td.double()) ** 2).mean()
        gY, = torch.autograd.grad(loss2, Yr)
        return {'dZ2': (gY * Y.double() * (1 - Y.double()), RTOL)}
    return run, ref


@case('gan_colsum')
def _(ops):
    gen = torch.Generator().manual_seed(111)
    A, Bm, wa, wb = randn(gen, 131, 1003), randn(gen, 131, 1003), randn(gen, 131), randn(gen, 131)
    return (lambda caller: {'plain': ops.gan_colsum(A), 'weighted': ops.gan_colsum(A, wa, Bm, wb), 'one': ops.gan_colsum(A[:1].contiguous())},
            lambda: {'plain': A.double().sum(0), 'weighted': (wa.double()[:, None] * A.double() + wb.double()[:, None] * Bm.double()).sum(0), 'one': A[0].double()})


@case('gan_threshold')
def _(ops):
    Y = torch.rand(37, 1003, generator=torch.Generator().manual_seed(112)).to(DEV)
    Y[0] = 0.0                                                            # an empty row
    Y0 = torch.zeros(5, 64, device=DEV)                                   # nothing above the threshold: nnz = 0

    def run(caller):
        rp, col = ops.gan_threshold(Y, 0.9)
        rp0, col0 = ops.gan_threshold(Y0, 0.9)
        return {'rp': rp, 'col': col, 'rp0': rp0, 'col0': col0}

    def ref():
        r, c = torch.nonzero(Y > 0.9, as_tuple=True)
        rp = torch.zeros(38, dtype=torch.float64, device=DEV); rp[1:] = torch.cumsum(torch.bincount(r, minlength=37), 0).double()
        return {'rp': (rp, 0.0), 'col': (c.double(), 0.0)}
    return run, ref


def template_inputs():
    gen = torch.Generator().manual_seed(113)
    U, I, F, S = 67, 131, 9, 46
    dense = (torch.rand(U, I, generator=gen) < 0.2).float() * torch.randint(1, 6, (U, I), generator=gen).float()
    dense[3] = 0
    rr, cc = dense.nonzero(as_tuple=True)
    rowptr = torch.zeros(U + 1, dtype=torch.int64); rowptr[1:] = torch.cumsum(torch.bincount(rr, minlength=U), 0)
    items = torch.randperm(I, generator=gen)[:S]
    pos = torch.full((I,), -1, dtype=torch.int64); pos[items] = torch.arange(S)
    user_set = torch.tensor([3, 0, 66, 5, 5, 17, 40, 41, 42])
    mask = (torch.rand(F, S, generator=gen) < 0.6).to(torch.uint8)
    item_p = torch.rand(I, generator=gen)
    dv = lambda t, dt: t.to(dt).to(DEV)
    return (dense, user_set, items, mask, dv(user_set, torch.int32), dv(rowptr, torch.int64), dv(cc, torch.int32), dense[rr, cc].to(DEV), dv(pos, torch.int32),
            dv(items, torch.int32), mask.to(DEV), item_p.to(DEV))


@case('gan_template')
def _(ops):
    dense, user_set, items, mask, us_d, rp_d, col_d, val_d, pos_d, items_d, mask_d, ip_d = template_inputs()

    def densify(rp, col, val):
        out = torch.zeros(len(user_set), len(items), dtype=torch.float64, device=DEV)
        rows = torch.repeat_interleave(torch.arange(len(user_set), device=DEV), rp[1:] - rp[:-1])
        out[rows, col.long()] = val.double()
        return out

    def run(caller):
        rp, col, val = ops.gan_template(us_d, rp_d, col_d, val_d, pos_d, items_d, mask=mask_d)
        rp2, col2, val2 = ops.gan_template(us_d, rp_d, col_d, val_d, pos_d, items_d, item_p=ip_d, seed=3, call=1)
        return {'rp': rp, 'col': col, 'val': val, 'dense': densify(rp, col, val), 'rp2': rp2, 'col2': col2, 'val2': val2}

    def ref():           # pattern: the sampled user's selected items; value: the interaction matrix read at (row r, position j), the reference's own indexing
        F, S = mask.shape
        return {'dense': (((dense[user_set][:, items] != 0).float() * dense[:F, :S] * mask.float()).double().to(DEV), 0.0)}
    return run, ref


@case('gan_hash_mask')
def _(ops):
    _, _, items, _, _, _, _, _, _, items_d, _, ip_d = template_inputs()

    def run(caller):
        return {'m': ops.gan_hash_mask(9, items_d, ip_d, seed=3, call=1)}

    def ref():
        rows = np.repeat(np.arange(9), len(items))
        keep = ops.gan_hash_keep(rows, np.tile(items.numpy(), 9), ip_d.cpu().numpy(), 3, 1)
        return {'m': (torch.from_numpy(keep.reshape(9, -1).astype(np.float64)).to(DEV), 0.0)}
    return run, ref


def fresh_pairs(rng, U, I, deg):
    u, i = random_graph(rng, U, I, deg)
    o = np.lexsort((i, u))
    return u[o].astype(np.int64), i[o].astype(np.int64)


@case('IncrementalBipartite')
def _(ops):
    rng = np.random.default_rng(114)
    U, F, I = 60, 4, 30
    u, i = fresh_pairs(rng, U, I, 5)
    fakes = []
    for s in (115, 116):
        r2 = np.random.default_rng(s)
        k = np.unique(r2.integers(0, F * I, 25))
        fakes.append((T(k // I), T(k % I)))
    X = randn(torch.Generator().manual_seed(117), U + F + I, 12)

    def run(caller):
        inc = ops.IncrementalBipartite(T(u), T(i), U, F, I)
        r = {}
        for j, (fu, fi) in enumerate(fakes):
            gph = inc.update(fu, fi)
            r['val%d' % j], r['col%d' % j], r['rp%d' % j], r['y%d' % j] = gph.val, gph.col, gph.rowptr, ops.spmm(gph, X)
        return r

    def ref():
        r = {}
        for j, (fu, fi) in enumerate(fakes):
            au, ai = np.concatenate([u, U + fu.cpu().numpy()]), np.concatenate([i, fi.cpu().numpy()])
            o = np.lexsort((ai, au))
            fresh = ops.bipartite_graph(T(au[o]), T(ai[o]), U + F, I)
            r['val%d' % j], r['col%d' % j], r['rp%d' % j] = (fresh.val.double(), 0.0), (fresh.col.double(), 0.0), (fresh.rowptr.double(), 0.0)
        return r
    return run, ref


@case('CSRGraph')
def _(ops):
    """The long-row plan's partial workspace (CSRGraph._struct) grows with the width: the same graph object at d = 12, then 256, then 12 again."""
    g = graph(ops)
    ins = [spmm_inputs(g, d, 118 + k)[0] for k, d in enumerate((12, 256, 12))]

    def run(caller):
        A = ops.CSRGraph(g.rowptr, g.col, g.val, DEV, chunk=32)
        r = {}
        for k, X in enumerate(ins):
            r['y%d' % k] = ops.spmm(A, X)
            if caller:
                poison_(A._partial)
        return r
    return run, lambda: {'y%d' % k: g.M @ X.double() for k, X in enumerate(ins)}


@case('BlockedPlan')
def _(ops):
    """Split-row workspace of the blocked plan (BlockedPlan.struct) reused at two widths, 128 then 64."""
    g = graph(ops)
    ins = [spmm_inputs(g, d, 121 + k)[0] for k, d in enumerate((128, 64, 128))]

    def run(caller):
        A = ops.CSRGraph(g.rowptr, g.col, g.val, DEV, chunk=32).enable_blocked(split=g.U, rows_per_wave=16, hub=24, col_block=64)
        r = {}
        for k, X in enumerate(ins):
            r['y%d' % k] = ops.spmm(A, X)
            if caller:
                for st in A.blocked.sets:
                    poison_(st.get('partial'))
        return r
    return run, lambda: {'y%d' % k: g.M @ X.double() for k, X in enumerate(ins)}


# ------------------------------------------------------------------------------------------------ the sweep
def introspected(source):
    """Public functions and classes of a module's source that allocate with the empty family or take a caller buffer."""
    tree = ast.parse(source)
    found = set()
    for node in tree.body:
        if not isinstance(node, (ast.FunctionDef, ast.ClassDef)) or node.name.startswith('_'):
            continue
        allocs = any(isinstance(n, ast.Attribute) and n.attr in ('empty', 'empty_like', 'empty_strided', 'new_empty') for n in ast.walk(node))
        params = isinstance(node, ast.FunctionDef) and any(a.arg in CALLER_PARAMS for a in node.args.args + node.args.kwonlyargs)
        if allocs or params:
            found.add(node.name)
    return found


def test_every_allocating_op_has_a_case(ops):
    source = inspect.getsource(ops)
    found = introspected(source)
    assert len(found) >= 40 and {'spmm_rows', 'cw_topk_term', 'gan_colsum', 'SfaStages', 'bpr_l2_partial'} <= found       # the introspection itself works
    missing = sorted(found - set(CASES))
    assert not missing, 'ops without a poisoned-memory case: %s' % missing
    assert all(hasattr(ops, name) for name in CASES), sorted(n for n in CASES if not hasattr(ops, n))
    # and the check does fail for a new op: the same introspection on the source plus one allocating function and one that takes a caller buffer
    grown = introspected(source + '\n\ndef brand_new_op(x):\n    return torch.empty_like(x)\n\n\ndef other_new_op(x, workspace=None):\n    return x\n')
    assert grown == found | {'brand_new_op', 'other_new_op'}
    assert sorted(grown - set(CASES)) == ['brand_new_op', 'other_new_op']


def held_to_float64(results, refs, name):
    for key, want in refs.items():
        want, tol, rowwise = (want + (False,))[:3] if isinstance(want, tuple) else (want, TOL, True)       # (ref, tol): max-norm only; (ref, tol, True): close()
        got = results[key]
        a, b = H(got).reshape(-1) if got.dim() == 0 else H(got), H(want).reshape(-1) if want.dim() == 0 else H(want)
        assert a.shape == b.shape, (name, key, a.shape, b.shape)
        if tol == 0.0:
            assert np.array_equal(a, b), (name, key)
        elif rowwise and a.ndim == 2 and a.shape[0] > 1:
            assert close(a, b, tol=tol), (name, key)
        else:
            assert rel_err(a, b) < tol, (name, key, rel_err(a, b))


@pytest.mark.parametrize('name', sorted(CASES))
def test_op_is_independent_of_scratch_memory(ops, name):
    run, ref = CASES[name](ops)
    clean, again = run(False), run(False)
    with poisoned_allocations():
        alloc = run(False)
    caller = run(True)
    torch.cuda.synchronize()
    assert not has_nan(clean), name
    refs = ref()
    held_to_float64(clean, refs, name)
    if compare(clean, again) == []:
        assert name not in NOT_BITWISE, '%s is bit-identical when clean: take it off the NOT_BITWISE list' % name
        assert compare(clean, alloc) == [], name
        assert compare(clean, caller) == [], name
    else:
        assert name in NOT_BITWISE, '%s differs between two clean runs: %s' % (name, compare(clean, again))
        for res in (alloc, caller):
            assert not has_nan(res), name
            held_to_float64(res, refs, name)


# ------------------------------------------------------------------------------------------------ "not read" contracts
def test_z_is_not_read_when_beta_is_zero_or_the_row_is_unflagged(ops):
    g, gb = graph(ops), graph(ops, True)
    for A in (g.A, gb.A):
        for d in (12, 64):
            X, Z, st, zf = spmm_inputs(g, d, 200 + d)
            nanZ = torch.full_like(Z, float('nan'))
            want = ops.spmm(A, X, 0.5)
            assert torch.equal(ops.spmm(A, X, 0.5, 0.0, nanZ, out=Pz(g.N, d)), want)
            assert torch.equal(ops.spmm_flagged(A, X, None, 0.5, 0.0, nanZ, None, out=Pz(g.N, d)), want)
            Zs = Z * zf[:, None]
            Zn = torch.where(zf[:, None] != 0, Z, nanZ)                        # NaN on every row whose flag byte is 0
            assert torch.equal(ops.spmm_flagged(A, X, None, 0.5, 2.0, Zn, zf, out=Pz(g.N, d)), ops.spmm_flagged(A, X, None, 0.5, 2.0, Zs, zf))
            a, b = [t.clone() for t in st], [t.clone() for t in st]
            ops.spmm_adam(A, X, 0.25, 0.5, Zs, *a, 0.005, 7, zflags=zf)
            ops.spmm_adam(A, X, 0.25, 0.5, Zn, *b, 0.005, 7, zflags=zf)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
            a, b = [t.clone() for t in st], [t.clone() for t in st]
            ops.spmm_adam(A, X, 0.25, 0.0, None, *a, 0.005, 7)
            ops.spmm_adam(A, X, 0.25, 0.0, nanZ, *b, 0.005, 7)
            assert all(torch.equal(x, y) for x, y in zip(a, b)) and not has_nan(b)
    Gs, flags, nz = flag_inputs(g, 64, 203)
    bits = torch.zeros((g.N + 31) // 32, dtype=torch.int32, device=DEV)
    ops.mark_bits_(bits, nz, True, g.N)
    Gn = torch.where(flags[:, None] != 0, Gs, torch.full_like(Gs, float('nan')))
    assert torch.equal(ops.spmm_flagged(g.A, Gs, bits, 1.0, 1.0, Gn, flags, out=Pz(g.N, 64)), ops.spmm_flagged(g.A, Gs, bits, 1.0, 1.0, Gs, flags))


def test_rows_from_leaves_the_rows_it_names_equal_to_the_unhinted_call(ops):
    g, gb = graph(ops), graph(ops, True)
    X = spmm_inputs(g, 64, 204)[0]
    for A in (g.A, gb.A):
        want = ops.spmm(A, X)
        for r in (g.U, 17):
            got = ops.spmm(A, X, out=Pz(g.N, 64), rows_from=r)
            assert torch.equal(got[r:], want[r:])                              # rows below r may stay unwritten: not compared


def test_poisoned_out_is_overwritten_not_read(ops):
    """An op that overwrites its out= (sfa_l1 with accumulate=False, tables_sum, normalize_rows_bwd, ngcf_combine, ngcf_dense_fwd, simgcl_perturb_rng)
    gives the same bits into a NaN-filled out as into a fresh one; the two sddmm forms accumulate, so a NaN in out stays a NaN."""
    gen = torch.Generator().manual_seed(205)
    X, w, r0 = randn(gen, 67, 100), torch.randint(0, 4, (67,), generator=gen).float().to(DEV), randn(gen, 100)
    numel = int(w.sum().item()) * 100
    loss, G = ops.sfa_l1(X, w, r0, numel)
    loss2, G2 = ops.sfa_l1(X, w, r0, numel, accumulate=False, out=Pz(67, 100))
    assert torch.equal(G, G2) and torch.equal(loss, loss2)
    base = randn(gen, 67, 100)
    _, G3 = ops.sfa_l1(X, w, r0, numel, accumulate=True, out=base.clone())
    assert close(H(G3), H(base) + H(G), tol=TOL)                                # and accumulate=True does read it
    tabs = [randn(gen, 67, 12) for _ in range(3)]
    assert torch.equal(ops.tables_sum(tabs, 0.5, out=Pz(67, 12)), ops.tables_sum(tabs, 0.5))
    Y, nrm = ops.normalize_rows(X)
    assert torch.equal(ops.normalize_rows_bwd(Y, nrm, base, out=Pz(67, 100)), ops.normalize_rows_bwd(Y, nrm, base))
    Pm, E = randn(gen, 67, 64), randn(gen, 67, 64)
    W = randn(gen, 128, 64, scale=0.3)
    assert torch.equal(ops.ngcf_combine(Pm, E, out=Pz(67, 128)), ops.ngcf_combine(Pm, E))
    assert torch.equal(ops.ngcf_dense_fwd(Pm, E, W, out=Pz(67, 64)), ops.ngcf_dense_fwd(Pm, E, W))
    assert torch.equal(ops.simgcl_perturb_rng(X, 0.1, 7, 3, out=Pz(67, 100)), ops.simgcl_perturb_rng(X, 0.1, 7, 3))
    # the two sddmm forms ACCUMULATE into out (zeros when omitted): a NaN there must stay a NaN -- the contract is "read", stated the other way round
    g = graph(ops)
    dY, Xs = randn(gen, g.N, 12), randn(gen, g.N, 12)
    assert bool(torch.isnan(ops.sddmm_csr(g.A, dY, Xs, out=Pz(len(g.col)))).all())
    rows = torch.tensor([0, 5, 5], dtype=torch.int32, device=DEV)
    for d in (12, 64):                                                       # 64: the kernel of its own for that width
        dYd, Xd = randn(gen, g.N, d), randn(gen, g.N, d)
        assert bool(torch.isnan(ops.sddmm_rows_dense(dYd, Xd, rows, g.U, g.I, out=Pz(3, g.I))).all())
        base3 = randn(gen, 3, g.I)
        want = base3.double() + dYd.double()[rows.long()] @ Xd.double()[g.U:].T
        assert close(H(ops.sddmm_rows_dense(dYd, Xd, rows, g.U, g.I, out=base3.clone())), H(want), tol=TOL)


# ------------------------------------------------------------------------------------------------ workspaces that outlive a call: B after A = B alone
def test_fake_block_workspace_reused_between_calls(ops):
    A_, B_ = fb_inputs(130, 301, 64, 300), fb_inputs(7, 1345, 100, 301)
    B2 = fb_inputs(130, 301, 64, 302)                                          # same cache key as A_, other data
    for first, second in ((A_, B_), (A_, B2)):
        ops._FB_WS.clear()
        alone = ops.fake_block_rows_(second[0], second[1], second[2].clone(), second[5], 0.5)
        alone_c = ops.fake_block_cols_(second[0], second[4], second[3].clone(), second[6], 0.5)
        ops._FB_WS.clear()
        ops.fake_block_rows_(first[0], first[1], first[2].clone(), first[5], 0.5)
        for ws in ops._FB_WS.values():
            poison_(ws)
        assert torch.equal(ops.fake_block_rows_(second[0], second[1], second[2].clone(), second[5], 0.5), alone)
        assert torch.equal(ops.fake_block_cols_(second[0], second[4], second[3].clone(), second[6], 0.5), alone_c)


def test_cw_workspace_reused_between_calls(ops):
    A_ = cw_problem(*CW_SHAPES[2], seed=310)
    same_key = cw_problem(*CW_SHAPES[2], seed=311)
    other = cw_problem(*CW_SHAPES[0], seed=312)
    for second in (same_key, other):
        ops._CW_WS.clear()
        alone = ops.cw_topk_term(*second)
        ops._CW_WS.clear()
        ops.cw_topk_term(*A_)
        for ws in ops._CW_WS.values():
            poison_(ws)
        assert compare(alone, ops.cw_topk_term(*second)) == []


def exit_tables(U, I, d, masked, lone, seed):
    """Tables on which the early-exit build of the item stream is picked (stage_sufmax_kernel): items along +e1 whose norms fall from 2 to 1, then 600
    items of norm 0.01 along -e1 at the end of the norm-ordered stream; users along +e1, whose lists are complete long before that tail.  lone: one
    user along -e1, whose best items ARE the tail -- its workgroup must stream to the end, so nothing is skipped.  Returns (Pu, Pi, rp, mc, order):
    order = the items by descending norm (int32), the table itself is shuffled."""
    rng = np.random.default_rng(seed)
    e1 = np.zeros(d); e1[0] = 1.0
    norms = np.concatenate([np.geomspace(2.0, 1.0, I - 600), np.full(600, 0.01)])
    sign = np.concatenate([np.ones(I - 600), -np.ones(600)])
    Pi = (norms[:, None] * (sign[:, None] * e1[None, :] + 0.05 * rng.standard_normal((I, d)))).astype(np.float32)
    Pi = Pi[rng.permutation(I)]
    Pu = (e1[None, :] + 0.05 * rng.standard_normal((U, d))).astype(np.float32)
    if lone:
        Pu[37] = (-e1 + 0.01 * rng.standard_normal(d)).astype(np.float32)
    order = np.argsort(-np.linalg.norm(Pi, axis=1), kind='stable').astype(np.int32)
    rp = mc = None
    if masked:
        cols = [np.unique(rng.choice(I, size=int(rng.integers(0, 12)), replace=False)).astype(np.int32) for _ in range(U)]
        cols[1] = np.unique(np.concatenate([cols[1], order[:5]])).astype(np.int32)          # some of the largest items masked
        rp, mc = T(np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int32)), T(np.concatenate(cols))
    return T(Pu), T(Pi), rp, mc, T(order)


@pytest.mark.parametrize('d', [64, 128])
@pytest.mark.parametrize('form', ['cold', 'warm', 'masked'])
def test_topk_exit_probe_state_from_another_call_does_not_change_the_result(ops, form, d):
    """score_mask_topk with a streamed item order launches the exit build and the plain build behind two gate words, and what a pass learnt (its
    counters, copied to a pinned host slot) decides which builds the NEXT call of that shape launches: ops._EXIT_PROBE outlives the call.  B after
    A = B alone, with A leaving B (a) in the 'off' state -- A's exit build was picked and skipped nothing, so B launches the plain build only -- and
    (b) in the probing state with A's probe consumed.  Everything A and B allocate is poisoned, the pinned slot included."""
    U, I, k, masked = 70, 5000, 20, form == 'masked'
    key = (U, I, d, k, masked)
    A_off = exit_tables(U, I, d, masked, True, 400 + d)
    A_probe = exit_tables(U, I, d, masked, False, 401 + d)
    B_ = exit_tables(U, I, d, masked, False, 402 + d)

    def call(tabs):
        Pu, Pi, rp, mc, order = tabs
        got = ops.score_mask_topk(Pu, Pi, k, rp, mc, item_order=order)
        if form == 'warm':
            got = ops.score_mask_topk(Pu, Pi, k, rp, mc, item_order=order, warm_idx=got[0])
        return got
    ops.reset_exit_probe()
    alone = call(B_)
    assert key in ops._EXIT_PROBE and ops._EXIT_PROBE[key]['off'] == 0          # the probe is engaged: the call ran in mode 1 and left a pending copy
    # float64: B's lists (values; the bar of test_score_mask_topk_early_exit_is_exact_...)
    Pu, Pi, rp, mc, _ = B_
    sc = Pu.double() @ Pi.double().T
    if masked:
        rows = torch.repeat_interleave(torch.arange(U, device=DEV), (rp[1:] - rp[:-1]).long())
        sc[rows, mc.long()] = -10e8
    rval = torch.topk(sc, k, dim=1)[0]
    assert float((alone[1].double() - rval).abs().max()) <= 2e-6 * float(rval.abs().max())
    assert torch.equal(call(B_)[1], alone[1]) and torch.equal(call(B_)[0], alone[0])       # bit-identical when clean
    ops.reset_exit_probe()
    with poisoned_allocations():
        assert compare(alone, call(B_)) == []                                  # B alone, poisoned
    for first, state in ((A_off, 'off'), (A_probe, 'probing')):
        ops.reset_exit_probe()
        with poisoned_allocations():
            ops.score_mask_topk(first[0], first[1], k, first[2], first[3], item_order=first[4])
            torch.cuda.synchronize()                                           # A's counters have reached the host slot: B's first call consumes them
            assert ops._EXIT_PROBE[key]['pending'] is not None
            after = call(B_)
        st = ops._EXIT_PROBE[key]
        if state == 'off':
            assert st['off'] > 0, 'A was meant to switch the exit build off for B (picked, nothing skipped)'
        else:
            assert st['off'] == 0 and st['pending'] is not None
        assert compare(alone, after) == [], state


def test_topk_exact_form_after_another_call_equals_alone(ops):
    """The exact fp32 form and the unordered stream keep no state between calls; B after A = B alone under poisoned allocations."""
    for masked in (False, True):
        A_, B_ = topk_problem(70, 1412, 64, masked, 320), topk_problem(70, 1412, 64, masked, 321)
        for kw in ({'exact': True}, {}):
            alone = ops.score_mask_topk(B_[0], B_[1], 20, B_[2], B_[3], **kw)
            with poisoned_allocations():
                ops.score_mask_topk(A_[0], A_[1], 20, A_[2], A_[3], **kw)
                assert compare(alone, ops.score_mask_topk(B_[0], B_[1], 20, B_[2], B_[3], **kw)) == []


def test_sfa_stages_reused_for_two_inputs(ops):
    gen = torch.Generator().manual_seed(330)
    X1, X2 = randn(gen, 777, 100), randn(gen, 777, 100)
    w, r0 = torch.randint(0, 4, (777,), generator=gen).float().to(DEV), randn(gen, 100)
    numel = int(w.sum().item()) * 100

    def stages(st):
        r = st.stage1(); a_s = st.stage2(r)
        return (r, a_s) + st.stage3(r, a_s, numel)
    alone = stages(ops.SfaStages(X2, w, r0))
    st = ops.SfaStages(X1, w, r0)
    stages(st)
    st.X = X2                                                                  # the same object (and workspace) for a second input
    assert compare(alone, stages(st)) == []
    poison_(st.ws)
    assert compare(alone, stages(st)) == []


# ------------------------------------------------------------------------------------------------ steps
def step_problem(seed=9, U=600, I=90, d=64, B=128):
    rng = np.random.default_rng(seed)
    us = np.repeat(np.arange(U), 10)
    its = np.floor(I * rng.random(len(us)) ** 2).astype(np.int64)
    key = np.unique(us * I + its)
    us, its = (key // I).astype(np.int32), (key % I).astype(np.int32)
    rowptr, col, w, val = make_csr(us, its, U, I)
    E0 = ((rng.random((U + I, d)) * 2 - 1) * 0.05).astype(np.float32)

    def batch(k, B=B):
        r = np.random.default_rng(seed * 100 + k)
        sel = r.integers(0, len(us), B)
        bu, bp, bn = us[sel].copy(), its[sel].copy(), r.integers(0, I, B).astype(np.int32)
        if B > 8:
            bu[:5] = bu[0]; bp[:6] = bp[1]; bn[:3] = bp[1]                    # duplicates; an item both positive and negative
        return T(bu), T(bp), T(bn)
    return U, I, d, (rowptr, col, val), E0, batch


def engine_state(eng):
    return {'E0': eng.E0.clone(), 'm': eng.m.clone(), 'v': eng.v.clone()}


def sparse_state_is_clean(eng):
    return (float(eng.G.abs().max()) == 0.0 and int(eng.flags.max()) == 0 and int(eng.bits.abs().max()) == 0 and int(eng.dup_bits.abs().max()) == 0)


def clean_and_poisoned(fn):
    """fn() run clean twice and once inside poisoned_allocations(); the section's rule on the three results."""
    a, b = fn(), fn()
    with poisoned_allocations():
        c = fn()
    torch.cuda.synchronize()
    assert not has_nan(a)
    return a, b, c


def assert_steps_match(name, a, b, c):
    if compare(a, b) == []:
        assert name not in NOT_BITWISE, name
        assert compare(a, c) == [], name
    else:
        assert name in NOT_BITWISE, '%s differs between two clean runs: %s' % (name, compare(a, b))
        assert not has_nan(c), name
        for (pa, x), (_, y) in zip(_leaves(a), _leaves(c)):
            assert rel_err(H(y), H(x)) < RTOL, (name, pa)


def _leaves(x, path='r'):
    if isinstance(x, dict):
        return [l for k in x for l in _leaves(x[k], path + '.' + str(k))]
    if isinstance(x, (list, tuple)):
        return [l for k, v in enumerate(x) for l in _leaves(v, '%s[%d]' % (path, k))]
    return [(path, x)] if isinstance(x, torch.Tensor) and x.is_floating_point() else []


@pytest.mark.parametrize('L', [1, 2, 3, 4])
@pytest.mark.parametrize('schedule', ['csr', 'blocked'])
def test_engine_sparse_and_dense_steps_under_poison(ops, L, schedule):
    from arlib_amd import engine
    U, I, d, (rowptr, col, val), E0, batch = step_problem()

    def run(kind):
        eng = engine.PropagationEngine(ops.CSRGraph(rowptr, col, val, DEV, chunk=64), U, I, d, L, 1e-4, 0.005, DEV, table=T(E0.copy()), schedule=schedule)
        losses = []
        for k in range(3):
            losses.append((eng.step if kind == 'sparse' else eng.step_dense)(*batch(k)).clone())
            if kind == 'sparse':
                assert sparse_state_is_clean(eng), (L, k)
        return {'losses': losses, **engine_state(eng)}
    for kind in ('sparse', 'dense'):
        assert_steps_match('engine.%s' % kind, *clean_and_poisoned(lambda: run(kind)))


def test_engine_state_machine_under_poison(ops):
    """Batch sizes B1, B2, B1 and then nine more distinct sizes (the per-size cache evicts past 8), then sparse / dense / sparse (the dirty-G path);
    G, flags, bits and dup_bits are all-zero after every sparse-form step; the whole sequence equals the same sequence run clean."""
    from arlib_amd import engine
    U, I, d, (rowptr, col, val), E0, batch = step_problem(seed=11)
    sizes = [128, 67, 128] + [3, 17, 33, 64, 65, 100, 129, 200, 255]

    def run():
        eng = engine.PropagationEngine(ops.CSRGraph(rowptr, col, val, DEV, chunk=64), U, I, d, 3, 1e-4, 0.005, DEV, table=T(E0.copy()), schedule='csr')
        losses = []
        for k, B in enumerate(sizes):
            losses.append(eng.step(*batch(k, B)).clone())
            assert sparse_state_is_clean(eng), (k, B)
        assert len(eng._sb_cache) == 8 and 128 not in eng._sb_cache             # evicted
        losses.append(eng.step(*batch(50, 128)).clone())                       # the evicted size again: fresh buffers
        assert sparse_state_is_clean(eng)
        losses.append(eng.step_dense(*batch(51)).clone())
        assert eng._G_dirty
        losses.append(eng.step(*batch(52)).clone())
        assert sparse_state_is_clean(eng) and not eng._G_dirty
        losses.append(eng.step_dense(*batch(53, 67)).clone())
        losses.append(eng.step(*batch(54, 67)).clone())
        assert sparse_state_is_clean(eng)
        return {'losses': losses, **engine_state(eng)}
    assert_steps_match('engine.state_machine', *clean_and_poisoned(run))


@pytest.mark.parametrize('which', ['ssl4rec', 'ngcf', 'simgcl', 'xsimgcl', 'sgl'])
def test_model_engine_steps_under_poison(ops, which):
    from arlib_amd import engine
    d = 16 if which in ('simgcl', 'xsimgcl') else 64
    U, I, _, (rowptr, col, val), E0, batch = step_problem(seed=13, d=d)
    L = 2
    gen = torch.Generator().manual_seed(14)
    masks = (torch.rand(3, 2, 2, 128, d, generator=gen) >= 0.2).to(DEV)
    noise = torch.rand(3, 2, L, U + I, d, generator=gen).to(DEV)
    W0 = [(randn(gen, d, d, scale=0.3), randn(gen, d, d, scale=0.3)) for _ in range(L)]
    keep = torch.rand(2, len(col), generator=gen) > 0.1                       # two edge-dropout views (symmetry is not needed for this comparison's sake)
    views_val = [torch.from_numpy(val) * keep[v] for v in range(2)]

    def run():
        A = ops.CSRGraph(rowptr, col, val, DEV, chunk=64)
        eng = engine.PropagationEngine(A, U, I, d, L, 1e-4, 0.005, DEV, table=T(E0.copy()), skip_layer0=which in ('simgcl', 'xsimgcl'))
        out = []
        if which == 'ngcf':
            Ws = [(a.clone(), b.clone()) for a, b in W0]
            eng.init_ngcf(Ws)
        if which == 'sgl':
            views = [A.with_values(v.to(DEV).contiguous()) for v in views_val]
        for k in range(3):
            u, p, n = batch(k)
            if which == 'ssl4rec':
                lo, cl = eng.step_ssl4rec(u, p, n, masks=masks[k])
                lo2, cl2 = eng.step_ssl4rec(u, p, n, seed=5, stream_id=k)          # and the in-kernel draw
                out += [lo2.clone(), cl2.clone()]
            elif which == 'ngcf':
                lo, cl = eng.step_ngcf(u, p, n), torch.zeros(1, device=DEV)
            elif which == 'simgcl':
                lo, cl = eng.step_simgcl(u, p, n, noises=[[noise[k, v, h] for h in range(L)] for v in range(2)])
            elif which == 'xsimgcl':
                lo, cl = eng.step_xsimgcl(u, p, n, noises=[noise[k, 0, h] for h in range(L)])
            else:
                lo, cl = eng.step_sgl(u, p, n, views[0], views[1])
            out += [lo.clone(), cl.clone()]
            assert sparse_state_is_clean(eng), (which, k)
        st = engine_state(eng)
        if which == 'ngcf':
            st['W'] = [w for pair in Ws for w in pair]
        return {'out': out, **st}
    assert_steps_match('engine.step_' + which, *clean_and_poisoned(run))


@pytest.mark.parametrize('which', ['NCF', 'WRMF'])
def test_model_steps_under_poison(which):
    import test_gpu_ncf, test_gpu_wrmf
    mod = test_gpu_ncf if which == 'NCF' else test_gpu_wrmf
    from arlib_amd.util.loss import bpr_l2_loss

    def run():
        rec = mod._fresh()
        model = rec.model.cuda()
        U, I = rec.data.user_num, rec.data.item_num
        opt = torch.optim.Adam(model.parameters(), lr=0.005)
        gen = torch.Generator().manual_seed(15)
        losses = []
        for s in range(3):
            bu, bp, bn = (torch.randint(0, hi, (257,), generator=gen).to(DEV) for hi in (U, I, I))
            out = model.forward_rows(torch.cat([bu, bp + U, bn + U]).to(torch.int32))
            B = bu.numel()
            loss = (bpr_l2_loss if which == 'NCF' else rec._batch_loss)(out[:B], out[B:2 * B], out[2 * B:], 1e-4)
            opt.zero_grad(); loss.backward(); opt.step()
            losses.append(loss.detach().clone())
        params = {n: p.detach().clone() for n, p in model.named_parameters()}
        moments = {n: opt.state[p]['exp_avg'].clone() for n, p in model.named_parameters() if p in opt.state}
        return {'losses': losses, 'params': params, 'm': moments}
    assert_steps_match('model.' + which, *clean_and_poisoned(run))


def test_aush_fused_gradients_under_poison():
    from arlib_amd.attack.Gray import _gan
    from test_gpu_aush import make_problem, modules

    def run():
        tpl, P = make_problem(37, 1003, 5, seed=16, empty_rows=(0,))
        G, D = modules(P, 1003)
        out = []
        for _ in range(3):
            out += list(_gan.fused_d_grads(G, D, tpl, 5)) + list(_gan.fused_g_grads(G, D, tpl, 5))
        return [t.clone() for t in out]
    assert_steps_match('aush.fused_grads', *clean_and_poisoned(run))

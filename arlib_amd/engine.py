"""Device-resident training engine for the GMF / LightGCN / SimGCL hot loop.

One `step()` is one iteration of the reference's inner loop (recommender/LightGCN.py:47-64, GMF.py:39-54):
full-graph propagation, BPR + L2 on the gathered batch rows, backward through the propagation and a dense
Adam (or SGD) update of both embedding tables -- as 2L SpMM launches, three small loss kernels and (for
Adam) no separate optimizer launch at all: the update is fused into the epilogue of the last backward hop.

HBM layout (all fp32, row-major, allocated once):
    E0  [N,d]  the two embedding tables as ONE buffer: users rows [0,U), items rows [U,N)   (torch.cat eliminated)
    m,v [N,d]  Adam moments
    S   [N,d]  running layer sum, becomes the propagated output `out` in place
    Ea,Eb [N,d] ping-pong hop buffers (forward hops, then backward Horner accumulators)
    G   [N,d]  dL/d(out): zero except <= 3B rows (scatter-added by the BPR kernel)
Backward uses the symmetry of the normalised adjacency (Horner form):
    acc = G; repeat L-1 times: acc = G + A acc;  dE0 = (G + A acc) / (L+1).
"""
import torch

from . import ops


def mean_adjacency_gradient(A, E0, G, L, s, out, noises=None, eps=0.1):
    """out[e] += dL/d(value of stored entry e of the symmetric graph A) for out_tables = s * sum of layers E_k (k >= 1 always in the sum), E_{k+1} = A E_k
    (+ a gradient-free perturbation when `noises` is given), from G = dL/d(out_tables): dE_L = s G, dE_k = s G + A dE_{k+1}, entry (i, j) receives
    sum_{k=0}^{L-1} <dE_{k+1}[i], E_k[j]>.  L - 1 forward hops, L - 1 backward hops, L products over the pattern (ops.sddmm_csr)."""
    if L == 0:
        return out
    E = [E0]
    for k in range(L - 1):
        nxt = ops.spmm(A, E[-1])
        if noises is not None:
            ops.simgcl_perturb_(nxt, noises[k], eps)
        E.append(nxt)
    G = G.contiguous()
    acc = G
    for j in range(L):
        ops.sddmm_csr(A, acc, E[L - 1 - j], s, out=out)
        if j < L - 1:
            acc = ops.spmm(A, acc, 1.0, 1.0, G)
    return out


class PropagationEngine:
    def __init__(self, graph, n_users, n_items, emb_size, n_layers, reg, lr, device, skip_layer0=False,
                 optimizer='adam', betas=(0.9, 0.999), eps=1e-8, table=None, schedule='auto'):
        self.A = graph
        self.U, self.I, self.d, self.L = int(n_users), int(n_items), int(emb_size), int(n_layers)
        self.N = self.U + self.I
        self.reg, self.lr, self.betas, self.eps = float(reg), float(lr), betas, eps
        self.skip0 = bool(skip_layer0)
        self.optimizer = optimizer
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ops._lib.ArlError('PropagationEngine needs a GPU device (no CPU fallback)')
        if graph is None and self.L > 0:
            raise ValueError('n_layers > 0 needs a graph')
        if graph is not None and graph.n_rows != self.N:
            raise ValueError('graph has %d rows, expected U+I=%d' % (graph.n_rows, self.N))
        if self.L > 0:
            ops._check_width(self.d, 'PropagationEngine')      # the propagation hops' widths: refused here, before any buffer or launch
        if self.skip0 and self.L < 1:
            raise ValueError('skip_layer0 needs n_layers >= 1')
        if schedule not in ('auto', 'csr', 'blocked'):
            raise ValueError("schedule must be 'auto', 'csr' or 'blocked'")
        # full-table hops: register-blocked schedule (ops.BlockedPlan) for large graphs at d = 64, row-per-group CSR kernel otherwise
        if schedule != 'csr':
            ops.auto_blocked(graph, emb_size, split=self.U, force=(schedule == 'blocked'))
        if graph is not None and graph.nnz >= ops.BLOCKED_MIN_NNZ:
            graph.enable_masked_order()              # flag-masked hops take the rows sorted by length
        z = lambda: torch.zeros(self.N, self.d, dtype=torch.float32, device=self.device)
        self.E0 = z() if table is None else table
        if self.E0.shape != (self.N, self.d) or self.E0.dtype != torch.float32 or not self.E0.is_contiguous():
            raise ValueError('table must be contiguous fp32 [U+I, d]')
        self.m, self.v, self.G = z(), z(), z()
        if self.L > 0:
            self.S, self.Ea, self.Eb = z(), z(), z()
        else:
            self.S = self.E0
        self.t = 0
        self.loss_out = torch.zeros(4, dtype=torch.float32, device=self.device)
        # state that later steps fill in (nothing below allocates device memory here)
        self._G_dirty = True                        # the sparse steps keep G all-zero between calls; dense users leave it dirty
        self._noise_seed, self._noise_stream = None, 0      # in-kernel noise (SimGCL family) / dropout masks (SSL4Rec): see _streams()
        self.nsplit = 32            # capacity of the row-subset hop's workspace, in pieces per batch row on average (rows are cut by length: ops.spmm_rows; cfg2 needs ~1.3)
        self.flags = self.bits = self.dup_bits = self.hops = None                                   # node-sized, _sparse_buffers()
        self._sparse_B, self._sb_cache = None, {}
        self.Gc = self.out_c = self.rows_ws = self.ar = self.arB = self._ws = None                 # batch-sized, _sparse_buffers()
        self._sgl_acc = self._sgl_hops = None       # step_sgl()
        self._apr_ws = {}                           # step_apr(): the adversarial kernel's workspace per batch size
        self.ngcf_W = self.ngcf_m = self.ngcf_v = None      # init_ngcf()

    # views with the reference's names
    @property
    def user_emb(self):
        return self.E0[:self.U]

    @property
    def item_emb(self):
        return self.E0[self.U:]

    def forward(self, noises=None, eps=0.1, out=None):
        """Propagated tables [N,d] (recommender/LightGCN.py:230-240; SimGCL.py:198-210 when skip_layer0).
        `noises`: optional list of L [N,d] tensors (SimGCL perturbed view, injected or from torch.rand)."""
        L, A = self.L, self.A
        if L == 0:
            return self.E0
        S = self.S if out is None else out
        if noises is None and not self.skip0:
            if L == 1:
                return ops.spmm(A, self.E0, 0.5, 0.5, self.E0, out=S)
            ops.spmm_layersum(A, self.E0, self.E0, S, self.Ea)
            cur, nxt = self.Ea, self.Eb
            for _ in range(L - 2):
                ops.spmm_layersum(A, cur, S, S, nxt)
                cur, nxt = nxt, cur
            s = 1.0 / (L + 1)
            return ops.spmm(A, cur, s, s, S, out=S)
        # SimGCL family: mean over hops 1..L, optional perturbation after each hop
        cur, nxt, x = self.Ea, self.Eb, self.E0
        for k in range(L):
            ops.spmm(A, x, out=cur)
            if noises is not None:
                ops.simgcl_perturb_(cur, noises[k], eps)
            if k == 0:
                if self.skip0:
                    S.copy_(cur)
                else:
                    torch.add(self.E0, cur, out=S)
            else:
                S.add_(cur)
            x, cur, nxt = cur, nxt, cur
        S.mul_(1.0 / (L if self.skip0 else L + 1))
        return S

    def backward_to_table(self, G, out=None):
        """dL/dE0 from dL/d(out) (= G, [N,d]) without touching the optimizer state."""
        L, A = self.L, self.A
        if L == 0:
            return G
        acc, dst = self._dense_hops(G)
        if self.skip0:
            return ops.spmm(A, acc, 1.0 / L, out=dst)
        s = 1.0 / (L + 1)
        return ops.spmm(A, acc, s, s, G, out=dst)

    def _dense_hops(self, G):
        """The first L-1 hops of the dense Horner backward, acc = G; acc = G + A acc, ping-pong over Ea / Eb.  Returns (acc, the buffer the
        last hop may write): that hop, with its scale and its share of G, is the caller's."""
        acc, bufs = G, (self.Ea, self.Eb)
        for k in range(self.L - 1):
            acc = ops.spmm(self.A, acc, 1.0, 1.0, G, out=bufs[k % 2])
        return acc, bufs[(self.L - 1) % 2]

    def adjacency_gradient(self, G, out=None, noises=None, eps=0.1):
        """dL/d(values of A) from dL/d(out) = G for out = mean of the layers E_k, E_{k+1} = A E_k (+ a perturbation that carries no gradient when
        `noises` is given: the SimGCL views, recommender/SimGCL.py:198-210): what autograd leaves in `sparse_norm_adj.grad` when the reference sets
        `sparse_norm_adj.requires_grad = True` (recommender/LightGCN.py:41-43,58-59; SimGCL.py:44-47,62-63).  With s = 1/(L+1) (layers 0..L) or
        1/L (skip_layer0: layers 1..L), dE_L = s G, dE_k = s G + A dE_{k+1} (A symmetric; k >= 1 is in the mean either way), the gradient on a
        stored entry (i, j) is sum_k <dE_{k+1}[i], E_k[j]>: L - 1 forward hops, L - 1 backward hops and L products over the pattern
        (ops.sddmm_csr), ACCUMULATED into `out` ([nnz] fp32, CSR order).  noises: the [hop] tables of the forward this gradient belongs to."""
        L, A = self.L, self.A
        if out is None:
            out = torch.zeros(A.col.numel(), dtype=torch.float32, device=G.device)
        return mean_adjacency_gradient(A, self.E0, G, L, 1.0 / L if self.skip0 else 1.0 / (L + 1), out, noises, eps)

    # ---- the propagated mean on a row subset, with its backward: the sparse-batch schedule of step() for callers that keep autograd and
    # their own optimiser (an extra loss term, an optimiser over one table only, gradient capture)
    def forward_rows(self, rows):
        """mean(E_0 .. E_L)[rows] (LightGCN): L-1 full hops and the last hop on the listed rows only.  rows: int32 node ids, duplicates allowed."""
        L, A = self.L, self.A
        if L == 0 or self.skip0 or L > 8:
            raise ValueError('forward_rows: LightGCN mean over layers 0..L with 1 <= L <= 8')
        n = rows.numel()
        self._sparse_buffers(max(n // 3, 1) if n % 3 == 0 else n)          # node-sized buffers (flags, bits, hops); batch-sized ones are not used here
        return self._mean_rows(A, self.hops, rows)

    def backward_rows(self, rows, g_rows):
        """dL/dE0 [N, d] from dL/d(forward_rows(rows)) = g_rows: scatter into the (all-zero) gradient table, flag-masked first hop, Horner
        over the remaining hops; the sparse state is cleared again before returning."""
        L, A = self.L, self.A
        s = 1.0 / (L + 1)
        self._begin_sparse(self._sparse_B)                      # the buffers forward_rows() left current
        self._set_rows(rows, g_rows.contiguous())
        acc, bits = self._masked_hops(A, self.hops)
        out = ops.spmm_flagged(A, acc, bits, s, s, self.G, self.flags)
        self._clear_rows(rows)
        return out

    # ---- the parts of the sparse-batch schedule, each written once; the step_* methods below are these plus their own losses and perturbations
    def _begin_sparse(self, B):
        """Every sparse step opens with this: the buffers for batch size B current, G all-zero (it stays so between sparse steps: each clears
        the rows it set; a dense step in between leaves it dirty)."""
        self._sparse_buffers(B)
        if self._G_dirty:
            self.G.zero_()
            self._G_dirty = False

    def _batch_rows(self, u, p, n):
        """Node ids of the BPR rows: [0,B) users, [B,2B) positives, [2B,3B) negatives."""
        return torch.cat([u, p + self.U, n + self.U])

    def _contrast_rows(self, u, p):
        """(node ids of the batch's unique users followed by its unique positive items, number of users among them): the InfoNCE rows."""
        uidx = torch.unique(u.long())
        iidx = torch.unique(p.long()) + self.U
        return torch.cat([uidx, iidx]).to(torch.int32), uidx.numel()

    def _streams(self, n):
        """(seed, first of n consecutive stream numbers) for this step's in-kernel random draws (SimGCL-family noise, SSL4Rec dropout masks; an
        engine runs one family or the other).  The seed is taken once from torch's global generator, by the first step that needs it."""
        if self._noise_seed is None:
            self._noise_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            self._noise_stream = 0
        first = self._noise_stream
        self._noise_stream += n
        return self._noise_seed, first

    def _mean_rows(self, graph, hops, rows, out=None, workspace=None):
        """mean(E_0 .. E_L)[rows] over `graph`: L-1 full hops into hops[0..L-2], the last hop on the listed rows only."""
        layers = [self.E0]
        for k in range(self.L - 1):
            layers.append(ops.spmm(graph, layers[-1], out=hops[k]))
        return ops.spmm_rows(graph, layers[-1], rows, layers, 1.0 / (self.L + 1), nsplit=self.nsplit, out=out, workspace=workspace, check_range=False)

    def _bpr_compact(self, out_c, B):
        """BPR + L2 on compact batch rows ([0,B) users, [B,2B) positives, [2B,3B) negatives of out_c): loss_out and the per-sample gradients Gc."""
        self.Gc.zero_()
        ops.bpr_l2_fwd_bwd(out_c, B, self.ar, self.ar, self.arB, self.reg, self.Gc, workspace=self._ws, loss_out=self.loss_out, check_range=False, distinct_rows=True)

    def _set_rows(self, rows, grad):
        ops.batch_rows_set_(self.G, self.flags, self.bits, rows, grad, 1.0, check_range=False, dup_bits=self.dup_bits)      # duplicates accumulate in order; rows marked

    def _mark_rows(self, rows):
        ops.mark_rows_(self.flags, rows, 1, check_range=False)
        ops.mark_bits_(self.bits, rows, True, self.N, check_range=False)

    def _clear_rows(self, rows):
        ops.batch_rows_clear_(self.G, self.flags, self.bits, rows, check_range=False, dup_bits=self.dup_bits)

    def _masked_hops(self, graph, bufs, src=None, after_hop=None):
        """The first L-1 hops of the masked Horner backward over the rows set / marked in G: acc = src (G itself unless given); acc = G + A acc,
        the first hop gathering flagged rows only (bits), G read through the flags everywhere, hop k written to bufs[k % len(bufs)] (one buffer
        per hop, or two that take turns).  after_hop(level, acc): called after the hop that produced level L-1 .. 1 (XSimGCL's injection).
        Returns (acc, xflags) for the LAST hop, which is the caller's: with L == 1 that is still (src, bits)."""
        acc, bits = self.G if src is None else src, self.bits
        for k in range(self.L - 1):
            acc = ops.spmm_flagged(graph, acc, bits, 1.0, 1.0, self.G, self.flags, out=bufs[k % len(bufs)])
            bits = None
            if after_hop is not None:
                after_hop(self.L - 1 - k, acc)
        return acc, bits

    def loss_and_grad_out(self, out, u, p, n):
        self.G.zero_()
        self._G_dirty = True          # the sparse step keeps G all-zero between calls; dense users leave it dirty
        if self._ws is None or self._ws.numel() < 4 * u.numel():
            self._ws = torch.empty(4 * u.numel(), dtype=torch.float32, device=self.device)
        ops.bpr_l2_fwd_bwd(out, self.U, u, p, n, self.reg, self.G, workspace=self._ws, loss_out=self.loss_out, check_range=False)
        return self.loss_out

    def grad(self, u, p, n):
        """(loss_out, dL/dE0) for one batch; no parameter update."""
        out = self.forward()
        lo = self.loss_and_grad_out(out, u, p, n)
        return lo, self.backward_to_table(self.G)

    def step(self, u, p, n, rows=None):
        """One training iteration on a device batch (int32 tensors, already range-checked by the caller).
        Returns the device tensor [bpr, reg_term, ||U_b||, ||P_b||]; loss = [0]+[1] (no host sync here).

        Sparse-batch form (LightGCN + Adam): the loss reads the propagated table on <= 3B rows only and its gradient G is
        non-zero on those rows only, so
          * the last forward hop is evaluated on the batch rows alone (arl_spmm_csr_rows_f32), and the running layer sum
            is never materialised for the other N - 3B rows;
          * the first backward hop A.G gathers only edges whose source row is flagged (arl_spmm_csr_flagged_f32);
          * G is kept all-zero between steps (batch rows are cleared afterwards) instead of memset per step.
        Same numbers as `step_dense` (which evaluates all 2L hops on the full graph), 2 of the 2L full hops cheaper.
        `rows` = cat(u, U+p, U+n) may be passed in when the caller has it precomputed."""
        if self.optimizer != 'adam' or self.L == 0 or self.skip0 or self.L > 8:
            return self.step_dense(u, p, n)
        return self._step_sparse(u, p, n, rows, None)

    def _step_sparse(self, u, p, n, rows, extra_grad):
        """step()'s sparse-batch form; extra_grad(): adds a further loss's gradient into the compact rows Gc after the BPR kernel (SSL4Rec)."""
        L, A = self.L, self.A
        B = u.numel()
        if rows is None:
            rows = self._batch_rows(u, p, n)
        self._begin_sparse(B)
        s = 1.0 / (L + 1)
        # forward: L-1 full hops, last hop on the batch rows; loss + compact per-sample gradients
        self._mean_rows(A, self.hops, rows, out=self.out_c, workspace=self.rows_ws)
        self._bpr_compact(self.out_c, B)
        if extra_grad is not None:
            extra_grad()
        self._set_rows(rows, self.Gc)
        # backward (Horner): first hop gathers flagged rows only; G is read through the flags everywhere; Adam is the last hop's epilogue
        self.t += 1
        acc, bits = self._masked_hops(A, self.hops)
        if L == 1:
            ops.spmm_flagged(A, acc, bits, s, s, self.G, self.flags, out=self.hops[0])
            ops.adam_dense(self.E0, self.hops[0], self.m, self.v, self.lr, self.t, self.betas, self.eps)
        else:
            ops.spmm_adam(A, acc, s, s, self.G, self.E0, self.m, self.v, self.lr, self.t, self.betas, self.eps, zflags=self.flags)
        self._clear_rows(rows)
        return self.loss_out

    def step_ssl4rec(self, u, p, n, cl_rate=1.0, tau=0.2, drop=0.2, masks=None, seed=None, stream_id=None):
        """One SSL4Rec training iteration (recommender/SSL4Rec.py:58-75, 213-247): the step() schedule (LightGCN mean over layers 0..L, BPR + L2,
        Adam fused into the last backward hop) plus ONE call of the dropout-view InfoNCE kernel, which adds cl_rate * its gradient into the
        compact gradient rows [0, B) (users) and [B, 2B) (positives) before they enter G -- the contrastive term reads the same propagated
        batch rows as the BPR loss, so it costs no extra hop.  masks: optional bool [2 sides][2 views][B][d] (parity tests); default: drawn
        inside the kernel from a seed taken once from torch's global generator and a running stream number (one per step), or from the
        caller's (seed, stream_id).  Returns (loss_out, cl_loss) device tensors (no host sync)."""
        L, A = self.L, self.A
        if self.optimizer != 'adam' or self.skip0 or L < 1 or L > 8:
            raise ValueError('step_ssl4rec needs a LightGCN-mean engine (no skip_layer0, 1 <= L <= 8) with Adam')
        B = u.numel()
        if self.d not in ops.SSL_NCE_WIDTHS:
            raise ValueError('step_ssl4rec: embedding size %d unsupported (d in %s)' % (self.d, ops.SSL_NCE_WIDTHS))
        if masks is not None and tuple(masks.shape) != (2, 2, B, self.d):
            raise ValueError('step_ssl4rec: masks [2, 2, B, d]')
        if seed is None:
            seed, stream_id = self._streams(1)
        cl = []
        def contrastive():
            loss, _ = ops.ssl_dropout_nce(self.out_c[:B], self.out_c[B:2 * B], drop, tau, G=(self.Gc[:B], self.Gc[B:2 * B]), upstream=cl_rate,
                                          seed=seed, stream_id=stream_id, masks=masks)
            cl.append(loss)
        self._step_sparse(u, p, n, None, contrastive)
        cl = cl[0]
        return self.loss_out, cl_rate * (cl[1] + cl[0])

    def step_apr(self, u, p, n, eps=0.5, adv_reg=1.0):
        """One APR training iteration (Adversarial Personalized Ranking, He et al., SIGIR'18): the step() schedule plus ONE call of the
        adversarial-BPR kernel (ops.bpr_adv_fwd_bwd), which perturbs the rows the scorer reads by eps * l2_normalize(their BPR gradient, summed
        per node) and adds adv_reg * the gradient of BPR on the perturbed rows.  Sparse form: the kernel reads the compact propagated batch
        rows out_c and adds into the compact gradient Gc before it enters G -- no extra hop.  Dense form (L = 0: APR as published; SGD,
        skip_layer0, L > 8): step_dense with the kernel adding into G after the BPR kernel.  The L2 term stays on the clean rows.
        Returns (loss_out, adv_loss) device tensors (no host sync); loss = loss_out[0] + loss_out[1] + adv_reg * adv_loss."""
        B = u.numel()
        if not ops.bpr_adv_supported(B, self.d):
            raise ValueError('step_apr: batch size %d, embedding size %d unsupported (B <= %d, d <= %d)' % (B, self.d, ops.BPR_ADV_MAX_BATCH, ops.BPR_ADV_MAX_WIDTH))
        adv = torch.empty(2, dtype=torch.float32, device=self.device)
        ws = self._apr_ws.get(B)
        if ws is None:
            if len(self._apr_ws) >= 8:
                del self._apr_ws[next(iter(self._apr_ws))]
            ws = self._apr_ws[B] = torch.empty(ops._lib.lib().arl_bpr_adv_workspace_bytes(B, self.d) // 4, dtype=torch.float32, device=self.device)
        if self.optimizer != 'adam' or self.L == 0 or self.skip0 or self.L > 8:
            def adversarial(out):
                ops.bpr_adv_fwd_bwd(out, self.U, u, p, n, eps, G=self.G, upstream=adv_reg, workspace=ws, loss_out=adv, check_range=False)
            return self.step_dense(u, p, n, adversarial), adv_reg * adv[0]
        rows = self._batch_rows(u, p, n)
        def adversarial():
            ops.bpr_adv_fwd_bwd(self.out_c, B, self.ar, self.ar, self.arB, eps, groups=rows, G=self.Gc, upstream=adv_reg, workspace=ws, loss_out=adv,
                                check_range=False, distinct_rows=True)
        return self._step_sparse(u, p, n, rows, adversarial), adv_reg * adv[0]

    # ---- NGCF (recommender/NGCF.py:47-64,197-212): the whole training iteration without autograd or a torch optimizer.  Per layer ONE hop
    # P = A E (A(E W1) = (A E) W1) and the fp32-MFMA dense part (ops.ngcf_dense_*); sparse-batch schedule as in step(): the LAST layer is
    # evaluated on the <= 3B batch rows only (row-subset hop + a [3B, 2d] dense part), its backward re-enters the table through the flag-masked
    # hop; the Adam update of the tables is the epilogue of the last backward hop, the d x d weights get the dense Adam kernel.
    def init_ngcf(self, weights):
        """weights: [(W1_l, W2_l)] device tensors / Parameters, one pair per layer (updated in place by step_ngcf)."""
        if len(weights) != self.L or any(tuple(w.shape) != (self.d, self.d) for pair in weights for w in pair):
            raise ValueError('init_ngcf: one pair of [d, d] weights per layer')
        self.ngcf_W = [(a.data if hasattr(a, 'data') else a, b.data if hasattr(b, 'data') else b) for a, b in weights]
        z = lambda: torch.zeros(self.d, self.d, dtype=torch.float32, device=self.device)
        self.ngcf_m = [(z(), z()) for _ in weights]
        self.ngcf_v = [(z(), z()) for _ in weights]

    def step_ngcf(self, u, p, n, rows=None, slope=0.01, capture=None):
        """capture: optional dict; receives the table gradient ('table') and the weight gradients ('W') of this step (diagnostics / tests:
        the Adam update then runs as a separate dense launch instead of the last hop's epilogue -- same numbers)."""
        L, A, d = self.L, self.A, self.d
        if L < 1 or self.ngcf_W is None or d not in ops.NGCF_DENSE_WIDTHS:
            raise ValueError('step_ngcf: needs n_layers >= 1, init_ngcf() and d in %s' % (ops.NGCF_DENSE_WIDTHS,))
        B = u.numel()
        if rows is None:
            rows = self._batch_rows(u, p, n)
        self._begin_sparse(B)
        s = 1.0 / (L + 1)
        Wcat = [torch.cat([a, b], 0) for a, b in self.ngcf_W]
        # forward: L-1 full layers, the last one on the batch rows
        egos, Ps = [self.E0], []
        for l in range(L - 1):
            P = ops.spmm(A, egos[-1])
            Ps.append(P)
            egos.append(ops.ngcf_dense_fwd(P, egos[-1], Wcat[l], slope))
        # same edge-range split as the autograd route (NGCF._LastLayerRows): leaky_relu's derivative jumps at 0, so a pre-activation within
        # rounding of 0 can land on either side of the kink under a different summation order and change that row's gradient by ~1 % --
        # with one association for both routes they stay bit-identical (and both sit on the reference's side on its captured steps)
        P_r = ops.spmm_rows(A, egos[-1], rows, (), 1.0, nsplit=ops.ROWS_NSPLIT, check_range=False)
        E_r = ops.gather_rows(egos[-1], rows, check_range=False)
        out_r = ops.ngcf_dense_fwd(P_r, E_r, Wcat[L - 1], slope)
        acc = out_r + E_r
        for e in egos[:-1]:
            acc += ops.gather_rows(e, rows, check_range=False)
        acc *= s
        self._bpr_compact(acc, B)
        Gs = self.Gc * s                                         # every layer's batch rows receive this share of dL/d(out) directly
        # backward
        self.t += 1
        gP_r, gE_r, gW = ops.ngcf_dense_bwd(Gs, out_r, P_r, E_r, Wcat[L - 1], slope)
        gWs = [None] * L
        gWs[L - 1] = gW
        self._set_rows(rows, gP_r)
        g = ops.spmm_flagged(A, self.G, self.bits)              # A^T (rows' gP scattered) = A (...), A symmetric
        self._clear_rows(rows)
        ops.scatter_add_rows(g, rows, gE_r + Gs, 1.0, check_range=False)
        if L == 1:
            if capture is not None:
                capture['table'] = g.clone()
            ops.adam_dense(self.E0, g, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        for l in range(L - 2, -1, -1):
            gP, gE, gWs[l] = ops.ngcf_dense_bwd(g, egos[l + 1], Ps[l], egos[l], Wcat[l], slope)
            ops.scatter_add_rows(gE, rows, Gs, 1.0, check_range=False)
            if l > 0:
                g = ops.spmm(A, gP, 1.0, 1.0, gE)
            elif capture is not None:
                capture['table'] = ops.spmm(A, gP, 1.0, 1.0, gE)
                ops.adam_dense(self.E0, capture['table'], self.m, self.v, self.lr, self.t, self.betas, self.eps)
            else:
                ops.spmm_adam(A, gP, 1.0, 1.0, gE, self.E0, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        if capture is not None:
            capture['W'] = [w.clone() for w in gWs]
        for l in range(L):
            for k in range(2):
                ops.adam_dense(self.ngcf_W[l][k], gWs[l][k * d:(k + 1) * d], self.ngcf_m[l][k], self.ngcf_v[l][k], self.lr, self.t, self.betas, self.eps)
        return self.loss_out

    def step_simgcl(self, u, p, n, cl_rate=0.2, tau=0.2, eps=0.1, noises=None):
        """One SimGCL training iteration (recommender/SimGCL.py:51-63,198-219) on the sparse-batch schedule.

        Reference: 3 forwards (clean + two perturbed views) of L hops each and autograd through all of them = 6L full-graph
        hops.  Here:
          * hop 1 (A E0) is shared by the three forwards (the perturbation is added after it);
          * every forward's last hop is only consumed on batch rows (BPR rows; InfoNCE rows are the unique batch users /
            positive items) -> row-subset hops;
          * the perturbation sign(E)*normalize(noise)*eps carries no gradient, so all three forwards have the SAME linear
            backward operator (1/L) sum_{k=1..L} A^k: the three sparse output gradients are summed first and ONE Horner pass
            (flag-masked first hop, Adam fused into the last) replaces three.
        L = 2: 2 full hops + 1 masked + 3 row-subset hops instead of 12 full hops.
        noises: optional [view][hop] full [N,d] tensors (parity tests); default: uniform noise drawn inside the perturbation kernel, one
        stream per hop and view (the reference's rand_like calls).  Returns (loss_out, cl_loss) device tensors."""
        if not self.skip0 or self.optimizer != 'adam':
            raise ValueError('step_simgcl needs a skip_layer0 engine with Adam')
        L, A = self.L, self.A
        B = u.numel()
        self._begin_sparse(B)
        inv = 1.0 / L
        rows = self._batch_rows(u, p, n)
        rows_cl, nu = self._contrast_rows(u, p)
        # noise: injected tables (parity tests) or, by default, drawn inside the perturbation kernel from a seed taken once from torch's global
        # generator and a running stream number -- one "draw" per hop and view like the reference's rand_like calls, but no [N, d] noise table,
        # no clone of the operand, and the compact last-hop rows get exactly the values a full-table draw would have given them
        rng_mode = noises is None
        if rng_mode:
            seed, stream0 = self._streams(2 * L)
        rnd = (lambda v, k: noises[v][k]) if noises is not None else None
        def perturb_full(src, v, k, out=None):                          # hop-k table of view v
            if rng_mode:
                return ops.simgcl_perturb_rng(src, eps, seed, stream0 + v * L + k, out=out)
            dst = src.clone() if out is None else out.copy_(src)
            return ops.simgcl_perturb_(dst, rnd(v, k), eps)
        def perturb_rows(src, v, k, sel):                               # compact rows `sel` of the hop-k table of view v, in place
            if rng_mode:
                return ops.simgcl_perturb_rng(src, eps, seed, stream0 + v * L + k, out=src, row_ids=sel)
            return ops.simgcl_perturb_(src, rnd(v, k)[sel.long()].contiguous(), eps)
        # ---- forwards
        E1 = ops.spmm(A, self.E0, out=self.hops[0])                       # shared first hop
        def finish(first, view):                                            # hops 2..L on table `first`; returns compact rows [rows_sel, d]
            sel = rows if view is None else rows_cl
            layers, cur = [first], first
            for k in range(1, L - 1):
                nxt = ops.spmm(A, cur)
                if view is not None:
                    perturb_full(nxt, view, k, out=nxt)
                layers.append(nxt); cur = nxt
            if L == 1:
                return ops.gather_rows(first, sel, check_range=False)
            if view is None:
                return ops.spmm_rows(A, cur, sel, layers, inv, nsplit=self.nsplit, check_range=False)
            last = ops.spmm_rows(A, cur, sel, (), 1.0, nsplit=self.nsplit, check_range=False)
            perturb_rows(last, view, L - 1, sel)
            for t in layers:
                last += ops.gather_rows(t, sel, check_range=False)
            return last * inv
        out_c = finish(E1, None)
        self._bpr_compact(out_c, B)
        ops.scatter_add_rows(self.G, rows, self.Gc, 1.0, check_range=False)
        views = []
        for v in (0, 1):
            E1p = perturb_full(E1, v, 0)
            views.append(finish(E1p, v))
        lu, du1, du2 = ops.infonce_fwd_bwd(views[0][:nu].contiguous(), views[1][:nu].contiguous(), tau)
        li, di1, di2 = ops.infonce_fwd_bwd(views[0][nu:].contiguous(), views[1][nu:].contiguous(), tau)
        cl_loss = cl_rate * (lu[0] + li[0])
        gcl = torch.cat([du1 + du2, di1 + di2], 0)                         # both views differentiate through the same operator
        ops.scatter_add_rows(self.G, rows_cl, gcl, cl_rate, check_range=False)
        allrows = torch.cat([rows, rows_cl])
        self._mark_rows(allrows)
        # ---- one backward pass: acc = G; (L-1) x: acc = G + A acc; g = A acc / L
        self.t += 1
        acc, bits = self._masked_hops(A, (self.hops[1], self.hops[0]))
        if L == 1:      # the only hop gathers the sparse G itself
            tmp = ops.spmm_flagged(A, acc, bits, inv, 0.0, None, None, out=self.hops[1])
            ops.adam_dense(self.E0, tmp, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        else:
            ops.spmm_adam(A, acc, inv, 0.0, None, self.E0, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        self._clear_rows(allrows)
        return self.loss_out, cl_loss

    def step_xsimgcl(self, u, p, n, cl_rate=0.2, tau=0.1, eps=0.1, layer_cl=1, noises=None):
        """One XSimGCL training iteration (recommender/XSimGCL.py:62-75,205-223): ONE perturbed forward; BPR + L2 on the mean of
        layers 1..L; InfoNCE (temperature tau) between that mean and the layer-`layer_cl` output at the batch's unique users and
        unique positive items.  Sparse-batch schedule: L-1 full hops + a row-subset hop forward; backward
            acc_L = c_L,  acc_k = c_k + A acc_{k+1},  dE0 = A acc_1,   c_k = G_mean / L + [k == layer_cl] G_cl
        with the first hop gathering flagged rows only and Adam fused into the last (default L=2: 2 full hops in all).
        noises: optional [hop] full [N,d] tensors (parity tests); default: uniform noise drawn inside the perturbation kernel, one stream
        per hop (the reference's rand_like).  Returns (loss_out, cl_loss)."""
        if not self.skip0 or self.optimizer != 'adam':
            raise ValueError('step_xsimgcl needs a skip_layer0 engine with Adam')
        L, A = self.L, self.A
        if not (1 <= layer_cl <= L):
            raise ValueError('layer_cl must be in [1, L]')
        B = u.numel()
        self._begin_sparse(B)
        inv = 1.0 / L
        rows = self._batch_rows(u, p, n)
        rows_cl, nu = self._contrast_rows(u, p)
        sel = torch.cat([rows, rows_cl])                                    # compact rows: [0,3B) BPR, then the CL rows
        rng_mode = noises is None                                           # default: noise drawn inside the perturbation kernel (step_simgcl)
        if rng_mode:
            seed, stream0 = self._streams(L)
        # ---- forward
        layers, cur = [], self.E0
        for k in range(L - 1):
            nxt = ops.spmm(A, cur, out=self.hops[k] if L <= 3 else None)
            if rng_mode:
                ops.simgcl_perturb_rng(nxt, eps, seed, stream0 + k, out=nxt)
            else:
                ops.simgcl_perturb_(nxt, noises[k], eps)
            layers.append(nxt); cur = nxt
        last = ops.spmm_rows(A, cur, sel, (), 1.0, nsplit=self.nsplit, check_range=False)
        if rng_mode:
            ops.simgcl_perturb_rng(last, eps, seed, stream0 + L - 1, out=last, row_ids=sel)
        else:
            ops.simgcl_perturb_(last, noises[L - 1][sel.long()].contiguous(), eps)
        mean_c = last.clone()
        for t in layers:
            mean_c += ops.gather_rows(t, sel, check_range=False)
        mean_c *= inv
        cl_c = last[3 * B:] if layer_cl == L else ops.gather_rows(layers[layer_cl - 1], rows_cl, check_range=False)
        # ---- losses and compact gradients
        self._bpr_compact(mean_c[:3 * B].contiguous(), B)
        mcl = mean_c[3 * B:]
        lu, du1, du2 = ops.infonce_fwd_bwd(mcl[:nu].contiguous(), cl_c[:nu].contiguous(), tau)
        li, di1, di2 = ops.infonce_fwd_bwd(mcl[nu:].contiguous(), cl_c[nu:].contiguous(), tau)
        cl_loss = cl_rate * (lu[0] + li[0])
        g_mean_cl = torch.cat([du1, di1], 0)                                # w.r.t. the mean at the CL rows
        g_layer = torch.cat([du2, di2], 0) * cl_rate                        # w.r.t. the layer-`layer_cl` output at the CL rows
        # G <- G_mean / L  (sparse rows; G is all-zero between steps)
        ops.scatter_add_rows(self.G, rows, self.Gc, inv, check_range=False)
        ops.scatter_add_rows(self.G, rows_cl, g_mean_cl, cl_rate * inv, check_range=False)
        self._mark_rows(sel)
        # ---- backward: the masked Horner pass with G_cl added at level layer_cl
        self.t += 1
        src = self.G
        if layer_cl == L:                                                   # acc_L = G + G_cl: both sparse, on the same flagged rows ...
            if L > 1:                                                       # ... on a copy when later levels add G alone
                src = self.G.clone()
            ops.scatter_add_rows(src, rows_cl, g_layer, 1.0, check_range=False)
        def inject(level, acc):
            if level == layer_cl:
                ops.scatter_add_rows(acc, rows_cl, g_layer, 1.0, check_range=False)
        bufs = (self.hops[1], self.hops[0])
        acc, bits = self._masked_hops(A, bufs, src, inject)
        if L == 1:
            tmp = ops.spmm_flagged(A, acc, bits, 1.0, 0.0, None, None, out=bufs[0])
            ops.adam_dense(self.E0, tmp, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        else:
            ops.spmm_adam(A, acc, 1.0, 0.0, None, self.E0, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        self._clear_rows(sel)
        return self.loss_out, cl_loss

    def step_sgl(self, u, p, n, view1, view2, cl_rate=0.2, tau=0.2):
        """One SGL training iteration (recommender/SGL.py:54-64,231-256) on the sparse-batch schedule.  Three LightGCN passes --
        the clean graph for BPR + L2, two perturbed graphs (`view1`, `view2`: CSRGraphs of this epoch's edge/node dropout) for ONE
        InfoNCE over the batch's unique users and unique positive items -- each with L-1 full hops + a row-subset hop forward and a
        flag-masked first hop backward; the three table gradients are summed and applied by one dense Adam.  6(L-1) full hops
        instead of the 6L of three autograd passes.  Returns (loss_out, cl_loss)."""
        if self.skip0 or self.optimizer != 'adam' or self.L < 1:
            raise ValueError('step_sgl needs a LightGCN-style engine (layers 0..L averaged) with Adam')
        L = self.L
        B = u.numel()
        self._begin_sparse(B)
        s = 1.0 / (L + 1)
        rows = self._batch_rows(u, p, n)
        rows_cl, _ = self._contrast_rows(u, p)
        if self._sgl_acc is None:
            self._sgl_acc = torch.empty_like(self.E0)
            self._sgl_hops = [torch.empty_like(self.E0) for _ in range(max(L - 1, 1))]

        def backward_into(graph, sel, grad_c, accumulate):                  # _sgl_acc (+)= dL/dE0 of a pass whose output gradient is grad_c at rows sel
            self._set_rows(sel, grad_c)
            acc, bits = self._masked_hops(graph, self._sgl_hops)
            tmp = ops.spmm_flagged(graph, acc, bits, s, s, self.G, self.flags, out=self._sgl_hops[0] if L == 1 else self.hops[0])
            if accumulate:
                self._sgl_acc.add_(tmp)
            else:
                self._sgl_acc.copy_(tmp)
            self._clear_rows(sel)

        # clean pass: BPR + L2 on the batch rows
        out_c = self._mean_rows(self.A, self._sgl_hops, rows)
        self._bpr_compact(out_c, B)
        # the two views at the contrastive rows, one InfoNCE over users and items together
        v1 = self._mean_rows(view1, self._sgl_hops, rows_cl)
        v2 = self._mean_rows(view2, self._sgl_hops, rows_cl)
        lcl, d1, d2 = ops.infonce_fwd_bwd(v1, v2, tau)
        cl_loss = cl_rate * lcl[0]
        # backward: three passes into one gradient table, then Adam
        backward_into(self.A, rows, self.Gc, False)
        backward_into(view1, rows_cl, d1 * cl_rate, True)
        backward_into(view2, rows_cl, d2 * cl_rate, True)
        self.t += 1
        ops.adam_dense(self.E0, self._sgl_acc, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        return self.loss_out, cl_loss

    def _sparse_buffers(self, B):
        """Buffers of the sparse-batch step.  The node-sized ones exist once; the batch-sized ones are kept per batch size (an epoch has two:
        the full batches and the last one), so that the last batch of every epoch does not re-allocate them."""
        if self._sparse_B == B:
            return
        dev, d = self.device, self.d
        if self.flags is None:
            self.flags = torch.zeros(self.N, dtype=torch.uint8, device=dev)          # byte per row: read once per OUTPUT row (epilogue)
            self.bits = torch.zeros((self.N + 31) // 32, dtype=torch.int32, device=dev)   # bit per node: read once per EDGE (masked hop)
            self.dup_bits = torch.zeros_like(self.bits)                                   # rows a batch names more than once (ordered accumulation)
            # forward needs E_1..E_{L-1} alive at the same time; Ea/Eb cover L <= 3
            self.hops = [self.Ea, self.Eb] + [torch.empty_like(self.Ea) for _ in range(max(0, self.L - 3))]
        sb = self._sb_cache.get(B)
        if sb is None:
            ar = torch.arange(B, dtype=torch.int32, device=dev)
            sb = (torch.zeros(3 * B, d, dtype=torch.float32, device=dev), torch.empty(3 * B, d, dtype=torch.float32, device=dev),
                  torch.empty(3 * B * self.nsplit * d, dtype=torch.float32, device=dev), ar, ar + B, torch.empty(4 * B, dtype=torch.float32, device=dev))
            if len(self._sb_cache) >= 8:                   # unusual callers with many batch sizes: drop the oldest set
                del self._sb_cache[next(iter(self._sb_cache))]
            self._sb_cache[B] = sb
        self.Gc, self.out_c, self.rows_ws, self.ar, self.arB, self._ws = sb
        self._sparse_B = B

    def step_dense(self, u, p, n, extra_grad=None):
        """Reference-shaped step: all 2L hops over the full graph (kept for A/B comparison and for SGD / SimGCL / GMF).  extra_grad(out): adds a
        further loss's gradient into G after the BPR kernel (step_apr)."""
        L, A = self.L, self.A
        out = self.forward()
        lo = self.loss_and_grad_out(out, u, p, n)
        if extra_grad is not None:
            extra_grad(out)
        self.t += 1
        if self.optimizer == 'adam' and L > 0 and not self.skip0:
            acc, _ = self._dense_hops(self.G)
            s = 1.0 / (L + 1)
            ops.spmm_adam(A, acc, s, s, self.G, self.E0, self.m, self.v, self.lr, self.t, self.betas, self.eps)
            return lo
        g = self.backward_to_table(self.G)
        self.apply_grad(g)
        return lo

    def apply_grad(self, g):
        if self.optimizer == 'adam':
            ops.adam_dense(self.E0, g, self.m, self.v, self.lr, self.t, self.betas, self.eps)
        elif self.optimizer == 'sgd':
            ops.sgd_dense(self.E0, g, self.lr)
        else:
            raise ValueError('unknown optimizer %r' % (self.optimizer,))

    # --- accounting: algorithmic bytes of one train step
    def step_bytes(self, B):
        E, N, d, L = (self.A.nnz if self.A is not None else 0), self.N, self.d, self.L
        return L * (16 * E + 8 * N + 24 * N * d) + 28 * N * d + 24 * B * d

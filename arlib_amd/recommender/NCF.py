"""NCF -- mirror of the reference's recommender/NCF.py (class NCF :15-168, NCFEncoder :171-220) on the MI355X kernels.

The encoder keeps the reference's parameters (`_fc_layers`: Linear(d, 5d), Linear(5d, 2d), Linear(2d, d); `embedding_dict` with the MF and MLP
tables of users and items) and scores users and items at width 2d: [mf row | tower(mlp row)], tower = the three layers, each followed by ReLU.
The tower is one HIP kernel (ops.ncf_tower_fwd: exact fp32 MFMA, activations on chip) that writes the scored rows directly, so the reference's
two torch.cat cost nothing.  Widths outside ops.NCF_TOWER_WIDTHS take nn.Linear / ATen with the same semantics.
  * a training step evaluates the tower on the batch's 3B rows only (forward_rows, the rows form; the reference runs it on all U + I rows every
    step and reads 3B of them: same values, same gradients);
  * forward() under autograd runs the kernel over every row with its activations saved; without autograd the table form writes no activations.
The user and item tables of each kind are adjacent views of one [U + I, d] device buffer, so neither form copies a table.
"""
import torch
import torch.nn as nn

from .. import ops
from ._base import DEVICE, Recommender


class _Tower(torch.autograd.Function):
    """Scored rows [mf | tower(mlp)] of the listed rows (rows: int32, may repeat) or of every row (rows=None), forward and backward by kernel.
    Backward: the tower kernel's g_mlp rows and the mf half of the upstream gradient reach the tables through the ordered (atomic-free) row
    scatter; weight and bias gradients are the kernel's fixed-order sums."""

    @staticmethod
    def forward(ctx, user_mf, item_mf, user_mlp, item_mlp, W0, b0, W1, b1, W2, b2, enc, rows):
        mf, mlp = enc._pack()
        W = tuple(w.detach().contiguous() for w in (W0, b0, W1, b1, W2, b2))
        out, h1, h2 = ops.ncf_tower_fwd(mf, mlp, W, rows, save_activations=True, check_range=False)
        ctx.save_for_backward(out, h1, h2, *W)
        ctx.enc, ctx.rows, ctx.U = enc, rows, user_mf.shape[0]
        return out

    @staticmethod
    def backward(ctx, g_out):
        out, h1, h2, *W = ctx.saved_tensors
        g_out = g_out.contiguous()
        mf, mlp = ctx.enc._pack()
        N, d = mlp.shape
        rows, U = ctx.rows, ctx.U
        g_rows, gW = ops.ncf_tower_bwd(g_out, out, h1, h2, mlp, W, rows, check_range=False)
        if rows is None:
            g_mf, g_mlp = g_out[:, :d], g_rows
        else:
            g_mf = ops.scatter_add_rows(torch.zeros(N, d, dtype=torch.float32, device=mlp.device), rows, g_out[:, :d].contiguous(), 1.0, check_range=False)
            g_mlp = ops.scatter_add_rows(torch.zeros(N, d, dtype=torch.float32, device=mlp.device), rows, g_rows, 1.0, check_range=False)
        return (g_mf[:U], g_mf[U:], g_mlp[:U], g_mlp[U:], *gW, None, None)


class NCFEncoder(nn.Module):
    def __init__(self, data, emb_size, mlp_layer, sizes):
        super().__init__()
        self.data = data
        self.latent_size = emb_size
        self.mlp_layer = mlp_layer
        self.sizes = sizes
        self.in_out = [(self.sizes[i], self.sizes[i + 1]) for i in range(len(self.sizes) - 1)]
        # the reference's creation order (NCF.py:180-184): the three Linear layers draw from the CPU generator before the four tables
        self._fc_layers = torch.nn.ModuleList()
        for in_size, out_size in self.in_out:
            self._fc_layers.append(torch.nn.Linear(emb_size * in_size, emb_size * out_size))
        self.embedding_dict = self._init_model()

    def _init_model(self):
        initializer = nn.init.xavier_uniform_
        return nn.ParameterDict({
            'user_mf_emb': nn.Parameter(initializer(torch.empty(self.data.user_num, self.latent_size))),
            'item_mf_emb': nn.Parameter(initializer(torch.empty(self.data.item_num, self.latent_size))),
            'user_mlp_emb': nn.Parameter(initializer(torch.empty(self.data.user_num, self.latent_size))),
            'item_mlp_emb': nn.Parameter(initializer(torch.empty(self.data.item_num, self.latent_size))),
        })

    def attack_emb(self, users_emb_grad, items_emb_grad):
        with torch.no_grad():
            self.embedding_dict['user_mf_emb'] += users_emb_grad[:, :self.latent_size]
            self.embedding_dict['user_mlp_emb'] += users_emb_grad[:, self.latent_size:]
            self.embedding_dict['item_mf_emb'] += items_emb_grad[:, :self.latent_size]
            self.embedding_dict['item_mlp_emb'] += items_emb_grad[:, self.latent_size:]

    def _init_uiAdj(self, *args):
        raise Exception("This model hava no graph")

    # ---- device placement: each kind's user and item tables are adjacent views of one [U + I, d] buffer
    def _pack_kind(self, kind):
        u, i = self.embedding_dict['user_%s_emb' % kind], self.embedding_dict['item_%s_emb' % kind]
        U, d = u.shape
        ok = (u.is_cuda and i.is_cuda and u.is_contiguous() and i.is_contiguous() and i.data_ptr() == u.data_ptr() + U * d * u.element_size()
              and u.untyped_storage().data_ptr() == i.untyped_storage().data_ptr())
        if not ok:
            packed = torch.cat([u.data.to(DEVICE), i.data.to(DEVICE)], 0).contiguous()
            u.data, i.data = packed[:U], packed[U:]
        return torch.as_strided(u.data, (U + i.shape[0], d), (d, 1))

    def _pack(self):
        return self._pack_kind('mf'), self._pack_kind('mlp')

    def cuda(self, device=None):
        self._pack()
        for p in self._fc_layers.parameters():
            if not p.is_cuda:
                p.data = p.data.to(DEVICE)
        return self

    def _weights(self):
        return [t for lin in self._fc_layers for t in (lin.weight, lin.bias)]

    def _fused(self):
        return self.latent_size in ops.NCF_TOWER_WIDTHS and self.sizes == [1, 5, 2, 1]

    def _torch_tower(self, x):
        for lin in self._fc_layers:
            x = torch.relu(lin(x))
        return x

    def forward(self):
        self.cuda()
        e = self.embedding_dict
        U = self.data.user_num
        if not self._fused():
            mlp = self._torch_tower(torch.cat([e['user_mlp_emb'], e['item_mlp_emb']], 0))
            return torch.cat([e['user_mf_emb'], mlp[:U]], 1), torch.cat([e['item_mf_emb'], mlp[U:]], 1)
        params = [e['user_mf_emb'], e['item_mf_emb'], e['user_mlp_emb'], e['item_mlp_emb']] + self._weights()
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            out = _Tower.apply(*params, self, None)
        else:
            mf, mlp = self._pack()
            out = ops.ncf_tower_fwd(mf, mlp, tuple(w.detach() for w in self._weights()))
        return out[:U], out[U:]

    def forward_rows(self, rows):
        """Rows `rows` (int32 ids: users, then U + items) of forward()'s scored tables -- what a training step reads -- by the rows form."""
        self.cuda()
        e = self.embedding_dict
        if not self._fused():
            r = rows.long()
            mf, mlp = torch.cat([e['user_mf_emb'], e['item_mf_emb']], 0)[r], torch.cat([e['user_mlp_emb'], e['item_mlp_emb']], 0)[r]
            return torch.cat([mf, self._torch_tower(mlp)], 1)
        return _Tower.apply(e['user_mf_emb'], e['item_mf_emb'], e['user_mlp_emb'], e['item_mlp_emb'], *self._weights(), self, rows.contiguous())


class NCF(Recommender):
    def __init__(self, args, data):
        self._common_init(args, data, 'NCF')
        # Hyperparameter (NCF.py:27-29)
        self.mlp_layers = 2
        self.sizes = [1, 5, 2, 1]
        self.model = NCFEncoder(self.data, args.emb_size, self.mlp_layers, self.sizes)

    def _params(self):
        return list(self.model.parameters())

    def _fusable(self, optimizer):
        return None                          # no fused engine step: the caller's optimizer runs over the tables and the tower

    def _embgrad_begin(self, model):
        d2 = 2 * self.args.emb_size
        self.usergrad = torch.zeros((self.data.user_num, d2), device=DEVICE)
        self.itemgrad = torch.zeros((self.data.item_num, d2), device=DEVICE)

    def _embgrad_accumulate(self, model):
        e = model.embedding_dict
        self.usergrad += torch.cat([e['user_mf_emb'].grad, e['user_mlp_emb'].grad], 1)
        self.itemgrad += torch.cat([e['item_mf_emb'].grad, e['item_mlp_emb'].grad], 1)

    def _detached_forward(self):
        with torch.no_grad():
            u, i = self.model()
            return u.detach(), i.detach()

    def train(self, requires_adjgrad=False, requires_embgrad=False, gradIterationNum=10, Epoch=0, optimizer=None, evalNum=5):
        if requires_adjgrad and not requires_embgrad:
            self.model.sparse_norm_adj       # NCF.py:45: the encoder has no adjacency -> the reference's AttributeError, before any work
        return self._train_loop(Epoch, optimizer, evalNum, requires_embgrad=requires_embgrad, requires_adjgrad=requires_adjgrad,
                                gradIterationNum=gradIterationNum)

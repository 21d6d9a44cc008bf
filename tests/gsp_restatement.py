"""Float64 restatements for GSPAttack's tests, on dense matrices and in our own words: the all-pairs binary cross-entropy with its gradients, the
relaxed Gumbel top-k for given noise, and the repaired proxy with whole attack epochs (autograd in float64).  Nothing here touches the library."""
import numpy as np
import torch

EPS = 1e-7


def _sig(s):
    """(sigmoid(s), sigmoid(-s)) without rounding either from 1 - the other."""
    e = np.exp(-np.abs(s))
    t = 1.0 / (1.0 + e)
    return np.where(s >= 0, t, e * t), np.where(s >= 0, e * t, t)


def dense_targets(R, I, rowptr, col, val=None):
    """A [R, I] float64 with every listed entry's weight ADDED at its place (a repeated entry counts as often as it is listed)."""
    A = np.zeros((R, I))
    rows = np.repeat(np.arange(R), np.diff(np.asarray(rowptr)))
    np.add.at(A, (rows, np.asarray(col)), np.ones(len(rows)) if val is None else np.asarray(val, np.float64))
    return A


def bce_allpairs(Pu, Pi, A, rw, eps=EPS, upstream=1.0):
    """bce[r, i] = -(A log(sigmoid(s) + eps) + (1 - A) log(sigmoid(-s) + eps)), s = Pu Pi^T; rowloss = its row sums; loss = sum_r rw[r] rowloss[r];
    dPu, dPi = gradients of upstream * loss.  Returns (loss, rowloss, dPu, dPi)."""
    Pu, Pi, A, rw = (np.asarray(x, np.float64) for x in (Pu, Pi, A, rw))
    s = Pu @ Pi.T
    p, q = _sig(s)
    bce = -(A * np.log(p + eps) + (1 - A) * np.log(q + eps))
    rowloss = bce.sum(1)
    g = -(A * (p * q) / (p + eps) - (1 - A) * (p * q) / (q + eps)) * (upstream * rw)[:, None]
    return float((rw * rowloss).sum()), rowloss, g @ Pi, g.T @ Pu


def gumbel_topk_relaxed(x, k, noise, tau=1.0):
    """x [F, I] float64 tensor (may require grad), noise [k, F, I].  Returns (S, picks [F, k], gap): gap is the smallest difference, over all rounds
    and rows, between the largest and the second largest perturbed logit (x + m + g_r) / tau -- how close any pick came to going the other way."""
    m = torch.zeros_like(x)
    S = torch.zeros_like(x)
    picks, gap = [], float('inf')
    for r in range(k):
        z = (x + m + noise[r].to(x.dtype)) / tau
        top2 = torch.topk(z.detach(), 2, dim=1)[0]
        gap = min(gap, float((top2[:, 0] - top2[:, 1]).min()))
        S = S + torch.softmax(z, dim=1)
        j = torch.argmax(z.detach(), dim=1)
        m = m.scatter(1, j[:, None], float('-inf'))
        picks.append(j)
    return S, torch.stack(picks, 1), gap


def row_weights(R, I, batch=128):
    nb = -(-R // batch)
    n = np.full(R, float(batch))
    n[(nb - 1) * batch:] = R - (nb - 1) * batch
    return 1.0 / (nb * n * I)


def literal_batched_mean(bce, batch=128):
    """The reference's loop: the mean over batches of each batch's own mean (a torch tensor in, a torch scalar out)."""
    total, n = 0, 0
    for b in range(0, bce.shape[0], batch):
        total = total + bce[b:b + batch].mean()
        n += 1
    return total / n


def normalised_adjacency(A_real, S, degrees_from=None):
    """Dense A_hat [(R + I)^2] of the repaired proxy: users 0..R-1 (real, then fake), items R..R+I-1.  d^-1/2 is a constant taken from the block
    `degrees_from` (default: S.detach()), 0 for an empty node."""
    U, I = A_real.shape
    R = U + S.shape[0]

    def adjacency(block):
        top = torch.cat([A_real, block], 0)
        return torch.cat([torch.cat([torch.zeros(R, R, dtype=S.dtype), top], 1), torch.cat([top.t(), torch.zeros(I, I, dtype=S.dtype)], 1)], 0)
    rs = adjacency((S if degrees_from is None else degrees_from).detach()).sum(1)
    dinv = torch.where(rs > 0, rs.clamp_min(1e-300).pow(-0.5), torch.zeros_like(rs))
    return dinv[:, None] * adjacency(S) * dinv[None, :]


def proxy_forward(params, A_real, S):
    """params: dict user_emb [R, d], item_emb [I, d], w1 / w2 lists.  Returns (Pu [R, d], Pi [I, d]): the mean over the layers' tables."""
    Ahat = normalised_adjacency(A_real, S)
    E = torch.cat([params['user_emb'], params['item_emb']], 0)
    acc = E
    for W1, W2 in zip(params['w1'], params['w2']):
        P = Ahat @ E
        E = torch.nn.functional.leaky_relu((P + E) @ W1 + (P * E) @ W2, 0.01)
        acc = acc + E
    out = acc / (len(params['w1']) + 1)
    R = params['user_emb'].shape[0]
    return out[:R], out[R:]


def pair_logits(params, Pu_prev, Pi_prev, U):
    """x[f, i] = mlp(cat(Pu_prev[U + f], Pi_prev[i])), mlp = Linear - ReLU - Linear with torch's [out, in] weights."""
    F, I = Pu_prev.shape[0] - U, Pi_prev.shape[0]
    pairs = torch.cat([Pu_prev[U:, None, :].expand(F, I, -1), Pi_prev[None].expand(F, I, -1)], 2)
    h = torch.relu(pairs @ params['mlp_w0'].t() + params['mlp_b0'])
    return (h @ params['mlp_w1'].t() + params['mlp_b1'])[:, :, 0]


def epoch_loss(params, A_real, S, targets, alpha=1.0, beta=1.0, batch=128, eps=EPS):
    """alpha L_per + beta L_exPR for the block S; L_per is the literal batched mean over all R x I entries with the target matrix [A_real; S.detach()]."""
    Pu, Pi = proxy_forward(params, A_real, S)
    U = A_real.shape[0]
    s = Pu @ Pi.t()
    a = torch.cat([A_real, S.detach()], 0)
    bce = -(a * torch.log(torch.sigmoid(s) + eps) + (1 - a) * torch.log(torch.sigmoid(-s) + eps))
    L_per = literal_batched_mean(bce, batch)
    L_ex = (-torch.log(torch.sigmoid(s[U:][:, targets]) + eps)).mean()
    return alpha * L_per + beta * L_ex, Pu, Pi


def leaves(params):
    return [params['user_emb'], params['item_emb']] + list(params['w1']) + list(params['w2']) + [params[k] for k in ('mlp_w0', 'mlp_b0', 'mlp_w1', 'mlp_b1')]


def run_attack(params, A_real, targets, k, noises, lr=0.01, s_init=1e-4):
    """len(noises) epochs of the attack in float64 (torch.optim.Adam, stock arithmetic).  params: float64 leaf tensors with requires_grad.
    Returns dict(loss=[...], picks=[...], gap=smallest top-2 gap over all rounds and epochs, dS=first epoch's dLoss/dS, grads=first epoch's
    gradients by parameter name, S=[...])."""
    U, I = A_real.shape
    F = params['user_emb'].shape[0] - U
    opt = torch.optim.Adam(leaves(params), lr=lr)
    with torch.no_grad():
        Pu_prev, Pi_prev = proxy_forward(params, A_real, torch.full((F, I), s_init, dtype=torch.float64))
    out = dict(loss=[], picks=[], gap=float('inf'), dS=None, grads=None, S=[])
    for ep, noise in enumerate(noises):
        x = pair_logits(params, Pu_prev, Pi_prev, U)
        S, picks, gap = gumbel_topk_relaxed(x, k, noise)
        S.retain_grad()
        loss, Pu, Pi = epoch_loss(params, A_real, S, targets)
        opt.zero_grad()
        loss.backward()
        if ep == 0:
            out['dS'] = S.grad.detach().clone()
            out['grads'] = dict(w1=[w.grad.clone() for w in params['w1']], w2=[w.grad.clone() for w in params['w2']],
                                **{n: params[n].grad.clone() for n in ('user_emb', 'item_emb', 'mlp_w0', 'mlp_b0', 'mlp_w1', 'mlp_b1')})
        opt.step()
        Pu_prev, Pi_prev = Pu.detach(), Pi.detach()
        out['loss'].append(float(loss.detach())); out['picks'].append(picks.clone()); out['S'].append(S.detach().clone())
        out['gap'] = min(out['gap'], gap)
    return out

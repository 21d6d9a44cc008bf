"""Float64 restatement of the multinomial likelihood and of one Mult-VAE / Mult-DAE training step, in plain torch with hand-written gradients and no
import of the product.  Everything is dense: a test's shapes are a few hundred rows and items.

    z = q E^T,  lse_b = log sum_i exp z_bi,  n_b = sum_i A_bi  (A = the weights on the positives, 0 elsewhere),  p = softmax_i(z)
    nll[b] = n_b lse_b - sum_i A_bi z_bi
    dq[b]  = g_b (n_b sum_i p_bi E_i - sum_i A_bi E_i),     dE[i] = sum_b g_b (n_b p_bi - A_bi) q_b
and a row without positives gives nll = 0 and no gradient.

The step, for the batch's users `rows`, the per-edge keep flags `keep` (one per stored entry of the batch's profiles, row by row with ascending
items) and eps [B, d]:
    x~ = x / |x|_2,   x' = keep * x~ / (1 - dropout),   [mu | logvar] = x' W_enc + b_enc,   z = mu + eps exp(logvar / 2)   (DAE: z = mu)
    loss = mean_b nll_b(z, W_dec, x) + beta mean_b KL_b + reg (|W_enc|_F + |W_dec|_F),     KL_b = 1/2 sum_j (mu^2 + exp(logvar) - logvar - 1)."""
import torch

F64 = torch.float64


def softmax_nll(q, E, pos, w=None, g=None):
    """q [B, d], E [I, d], pos [B, I] bool, w [B, I] weights (read on the positives; None: 1), g [B] upstream (None: 1) -> nll, lse, dq, dE in float64."""
    q, E = q.to(F64), E.to(F64)
    A = pos.to(F64) if w is None else w.to(F64) * pos.to(F64)
    g = torch.ones(q.shape[0], dtype=F64) if g is None else g.to(F64)
    z = q @ E.t()
    lse = torch.logsumexp(z, 1)
    n = A.sum(1)
    has = pos.any(1).to(F64)
    nll = has * (n * lse - (A * z).sum(1))
    dz = (g * has)[:, None] * (n[:, None] * torch.softmax(z, 1) - A)
    return nll, lse, dz @ E, dz.t() @ q


def dense_profiles(X, rows, keep):
    """X [U, I] bool, rows [B] user ids, keep [nnz of X[rows]] -> (x [B, I] float64 binary, kept [B, I] float64: the keep flag on each stored entry)."""
    x = X[rows].to(F64)
    kept = torch.zeros_like(x)
    kept[x > 0] = keep.to(F64)                   # boolean-mask assignment runs row by row, ascending columns: the CSR order
    return x, kept


def step(W_enc, b_enc, W_dec, X, rows, keep, eps, beta, reg=0.0, dropout=0.5, variational=True):
    """One step's loss and gradients.  Returns a dict: loss, nll (mean), kl (mean), mu, and the gradients dW_enc, db_enc, dW_dec."""
    W_enc, b_enc, W_dec = W_enc.to(F64), b_enc.to(F64), W_dec.to(F64)
    d, B = W_dec.shape[1], len(rows)
    x, kept = dense_profiles(X, rows, keep)
    norm = x.sum(1).sqrt()
    xt = x / torch.where(norm > 0, norm, torch.ones_like(norm))[:, None]
    xin = kept * xt / (1.0 - dropout)
    h = xin @ W_enc + b_enc
    mu = h[:, :d]
    g = torch.full((B,), 1.0 / B, dtype=F64)
    if variational:
        logvar = h[:, d:]
        std = torch.exp(0.5 * logvar)
        z = mu + eps.to(F64) * std
        kl = 0.5 * (mu * mu + torch.exp(logvar) - logvar - 1.0).sum(1)
    else:
        z, kl = mu, torch.zeros(B, dtype=F64)
    nll, _, dz, dW_dec = softmax_nll(z, W_dec, x > 0, None, g)
    ne, nd = torch.linalg.norm(W_enc), torch.linalg.norm(W_dec)
    loss = nll.mean() + beta * kl.mean() + reg * (ne + nd)
    if variational:
        dmu = dz + (beta / B) * mu
        dlogvar = dz * eps.to(F64) * 0.5 * std + (beta / B) * 0.5 * (torch.exp(logvar) - 1.0)
        dh = torch.cat([dmu, dlogvar], 1)
    else:
        dh = dz
    dW_enc = xin.t() @ dh
    if reg:
        dW_enc = dW_enc + reg * W_enc / ne
        dW_dec = dW_dec + reg * W_dec / nd
    return {'loss': loss, 'nll': nll.mean(), 'kl': kl.mean(), 'mu': mu, 'dW_enc': dW_enc, 'db_enc': dh.sum(0), 'dW_dec': dW_dec}


def beta_at(t, vae_beta, anneal_steps):
    """The KL weight of the step taken after t completed steps."""
    return vae_beta * min(1.0, t / anneal_steps) if anneal_steps > 0 else vae_beta


def adam(params, grads, state, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam's update (no weight decay, no amsgrad) in float64, in place on `state` = {'t', 'm', 'v'}; returns the new parameters."""
    state['t'] += 1
    t, out = state['t'], []
    for k, (p, gr) in enumerate(zip(params, grads)):
        state['m'][k] = betas[0] * state['m'][k] + (1 - betas[0]) * gr
        state['v'][k] = betas[1] * state['v'][k] + (1 - betas[1]) * gr * gr
        mh = state['m'][k] / (1 - betas[0] ** t)
        out.append(p - lr * mh / ((state['v'][k] / (1 - betas[1] ** t)).sqrt() + eps))
    return out


def train_steps(W_enc, b_enc, W_dec, X, batches, lr, vae_beta, anneal_steps, reg=0.0, dropout=0.5, variational=True):
    """Steps over `batches` = [(rows, keep, eps), ...] with Adam from zero moments.  Returns the final (W_enc, b_enc, W_dec) and the steps' dicts."""
    P = [W_enc.to(F64).clone(), b_enc.to(F64).clone(), W_dec.to(F64).clone()]
    state = {'t': 0, 'm': [torch.zeros_like(p) for p in P], 'v': [torch.zeros_like(p) for p in P]}
    outs = []
    for t, (rows, keep, eps) in enumerate(batches):
        r = step(P[0], P[1], P[2], X, rows, keep, eps, beta_at(t, vae_beta, anneal_steps), reg, dropout, variational)
        outs.append(r)
        P = adam(P, [r['dW_enc'], r['db_enc'], r['dW_dec']], state, lr)
    return P, outs

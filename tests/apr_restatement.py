"""float64 numpy statement of APR's step (Adversarial Personalized Ranking, He et al., SIGIR'18) as arlib_amd defines it -- not a test.

Batch u, p, n [B]; positions t = b (user), B + b (positive), 2B + b (negative); position t reads row rows[t] = cat(u, p + off, n + off)[t] of the table
and belongs to node groups[t] (None: every position is its own group).  bpr(.) = mean(-log(10e-8 + sigmoid(<u,p> - <u,n>))).

  1. Gamma_g = sum over the positions of g, in ascending t, of d bpr / d(that position's row)
  2. delta_g = eps * Gamma_g / sqrt(max(|Gamma_g|^2, 1e-12)), a constant of the step
  3. adv     = bpr(e_u + delta[u], e_p + delta[p], e_n + delta[n])
  4. loss    = bpr + reg * (|e_u|_F + |e_p|_F) + adv_reg * adv           (L2 on the clean rows, un-squared)
"""
import numpy as np

EPS_LOG = 10e-8
NORM_FLOOR = 1e-12


def _bpr(eu, ep, en):
    """(loss, coefficient d loss / d x_b) of the mean BPR over rows [B, d]."""
    x = np.sum(eu * (ep - en), 1)
    s = 1.0 / (1.0 + np.exp(-x))
    return float(np.mean(-np.log(EPS_LOG + s))), -(s * (1.0 - s)) / ((EPS_LOG + s) * len(x))


def _position_grads(c, eu, ep, en):
    """d loss / d(row of position t), [3B, d], from the per-sample coefficients."""
    return np.concatenate([c[:, None] * (ep - en), c[:, None] * eu, -c[:, None] * eu], 0)


def batch_rows(u, p, n, item_off):
    return np.concatenate([np.asarray(u, np.int64), np.asarray(p, np.int64) + item_off, np.asarray(n, np.int64) + item_off])


def restate(emb, item_off, u, p, n, eps, groups=None, reg=0.0, adv_reg=1.0):
    """emb: [N, d] table (any float dtype; computed in float64).  Returns a dict:
    clean, adv, reg_term, loss      the terms and the step's loss
    delta  [3B, d]                  the perturbation each position receives
    cond   [3B]                     |Gamma_g| / sum |terms of g| of the position's group (1 = no cancellation; 0 where every term is 0)
    g_adv  [N, d]                   d adv / d emb, delta held constant, accumulated per row in position order
    g_loss [N, d]                   d loss / d emb"""
    E = np.asarray(emb, np.float64)
    rows = batch_rows(u, p, n, item_off)
    B = len(u)
    grp = np.arange(3 * B) if groups is None else np.asarray(groups, np.int64)
    _, gidx = np.unique(grp, return_inverse=True)
    e = E[rows]
    eu, ep, en = e[:B], e[B:2 * B], e[2 * B:]
    clean, c = _bpr(eu, ep, en)
    terms = _position_grads(c, eu, ep, en)
    Gamma = np.zeros((gidx.max() + 1, E.shape[1]))
    np.add.at(Gamma, gidx, terms)                                   # ascending position order
    tot = np.zeros(len(Gamma))
    np.add.at(tot, gidx, np.linalg.norm(terms, axis=1))
    nrm2 = np.sum(Gamma * Gamma, 1)
    delta = (eps * Gamma / np.sqrt(np.maximum(nrm2, NORM_FLOOR))[:, None])[gidx]
    adv, c2 = _bpr(eu + delta[:B], ep + delta[B:2 * B], en + delta[2 * B:])
    g_adv = np.zeros_like(E)
    np.add.at(g_adv, rows, _position_grads(c2, eu + delta[:B], ep + delta[B:2 * B], en + delta[2 * B:]))
    nu, npn = np.linalg.norm(eu), np.linalg.norm(ep)
    g_loss = adv_reg * g_adv
    np.add.at(g_loss, rows, terms)
    if nu > 0:
        np.add.at(g_loss, rows[:B], reg * eu / nu)
    if npn > 0:
        np.add.at(g_loss, rows[B:2 * B], reg * ep / npn)
    reg_term = reg * (nu + npn)
    cond = np.divide(np.sqrt(nrm2), tot, out=np.zeros_like(tot), where=tot > 0)[gidx]
    return {'clean': clean, 'adv': adv, 'reg_term': reg_term, 'loss': clean + reg_term + adv_reg * adv, 'delta': delta, 'cond': cond,
            'gamma_norm_sum': float(np.sqrt(nrm2).sum()), 'g_adv': g_adv, 'g_loss': g_loss}


def draw_case(B, d, users, items, seed):
    """N(0, 0.1) table and a batch with n != p per sample, as the sampler guarantees."""
    rng = np.random.default_rng(seed)
    E = rng.normal(0.0, 0.1, (users + items, d))
    u = rng.integers(0, users, B)
    p = rng.integers(0, items, B)
    n = (p + 1 + rng.integers(0, items - 1, B)) % items
    return E, u.astype(np.int32), p.astype(np.int32), n.astype(np.int32)


# the kernel shapes of tests/test_gpu_apr.py: (B, d, users, items, seed); with groups = the node ids every node of every case has cond >= 0.17
# (test_apr_cpu.py checks it: most seeds of the B = 7 shape do not, an item that is one user's positive and negative cancels)
CASES = [(1, 4, 3, 5, 11), (7, 4, 2, 3, 100), (86, 20, 9, 11, 13), (171, 64, 40, 60, 14), (2048, 64, 943, 1682, 15), (2048, 128, 943, 1682, 16),
         (5461, 64, 943, 1682, 17)]
COND_FLOOR = 1e-2

"""numpy float64 restatements of LegUP's ranking loss for the tests (no GPU, no library).

reference_expression: the reference's own formula (attack/Gray/LegUP.py:160-171), the [U, T, I] broadcast included.
colsoftmax_target_loss: the closed form arlib_amd.ops.colsoftmax_target computes, with its gradients:
    L = -(I sum_u sum_t s[u, c_t] - U T sum_i lse[i]),  lse[i] = log sum_u exp(s[u, i]),  s = Pu Pi^T
    dL/ds[u, i] = U T exp(s[u, i] - lse[i]) - I #{t : c_t = i}
"""
import numpy as np


def reference_expression(Pu, Pi, cols, dtype=np.float64):
    """-sum(log(exp(s[:, cols])[:, :, None] / sum_u exp(s))) with plain exp, in `dtype` (float32 shows where the reference overflows)."""
    s = (np.asarray(Pu, dtype) @ np.asarray(Pi, dtype).T).astype(dtype)
    with np.errstate(over='ignore', invalid='ignore', divide='ignore'):
        t = np.exp(s[:, list(cols)])[:, :, None]                    # [U, T, 1]
        return -np.sum(np.log(t / np.sum(np.exp(s), axis=0)))       # [U, T, I] broadcast


def colsoftmax_target_loss(Pu, Pi, cols, want_grad=False):
    """(loss, lse) or (loss, lse, dPu, dPi) in float64, log-sum-exp with the column maximum taken out."""
    Pu, Pi = np.asarray(Pu, np.float64), np.asarray(Pi, np.float64)
    cols = [int(c) for c in cols]
    U, I, T = Pu.shape[0], Pi.shape[0], len(cols)
    s = Pu @ Pi.T
    m = s.max(0)
    lse = m + np.log(np.exp(s - m).sum(0))
    loss = -(I * s[:, cols].sum() - U * T * lse.sum())
    if not want_grad:
        return loss, lse
    dS = U * T * np.exp(s - lse)
    for c in cols:
        dS[:, c] -= I
    return loss, lse, dS @ Pi, dS.T @ Pu

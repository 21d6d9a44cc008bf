"""Float64 restatements for PoisonRec and RLAttack, written from the formulas in the attacks' module docstrings and DESIGN.md section 3l, not from arlib_amd's code: the policy
head (log-probability, entropy, gradients by autograd, the sampling rule), GAE, the PPO loss with its KL stop, the repaired policy forward and one
environment step.  Used by test_poisonrec_cpu.py, test_ppo_cpu.py and the GPU tests."""
import numpy as np
import torch


# ------------------------------------------------------------------------------------------------ the head
def head(q, E, a, gl=None, ge=None):
    """q [B, d], E [I, d], a [B, I] of 0/1.  p = softmax_i(q E^T); logp = sum_i (a p - softplus(p)), ent = sum_i (softplus(p) - p sigmoid(p)) -- the
    log-probability and the entropy of Bernoulli(logits = p).  With gl, ge [B]: also the gradients of sum_b gl logp + ge ent by autograd.
    Returns (logp, ent, dq, dE, p)."""
    q, E, a = q.double().detach().requires_grad_(), E.double().detach().requires_grad_(), a.double()
    p = torch.softmax(q @ E.t(), dim=1)
    sp = torch.log1p(torch.exp(p))
    logp = (a * p - sp).sum(1)
    ent = (sp - p / (1 + torch.exp(-p))).sum(1)
    dq = dE = None
    if gl is not None:
        (gl.double() * logp + ge.double() * ent).sum().backward()
        dq, dE = q.grad, E.grad
    return logp.detach(), ent.detach(), dq, dE, p.detach()


def sample(q, E, u):
    """a_i = (u_i < sigmoid(p_i)): (a [B, I] bool, logp [B], count [B], the smallest |u - sigmoid(p)| met, sigmoid(p))."""
    p = torch.softmax(q.double() @ E.double().t(), dim=1)
    sg = 1 / (1 + torch.exp(-p))
    a = u.double() < sg
    logp = (a.double() * p - torch.log1p(torch.exp(p))).sum(1)
    return a, logp.detach(), a.sum(1), float((u.double() - sg).detach().abs().min()), sg.detach()


def pack(a):
    """[B, I] bool -> [B, ceil(I / 32)] int32: bit i % 32 of word i / 32 is item i, pad bits 0 (numpy, independent of arlib_amd.pack_bits)."""
    a = np.asarray(a).astype(bool)
    B, I = a.shape
    W = (I + 31) // 32
    bits = np.zeros((B, W * 32), np.uint64)
    bits[:, :I] = a
    words = (bits.reshape(B, W, 32) << np.arange(32, dtype=np.uint64)).sum(2).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32).copy())


# ------------------------------------------------------------------------------------------------ GAE and the PPO loss
def gae(rewards, values, episode_starts, last_value, last_done, gamma, lam):
    """Generalised advantage estimation over one rollout of n steps (lists or arrays of floats).  episode_starts[t] is 1 when step t begins an episode;
    last_done is 1 when the step after the rollout begins one (its bootstrap value is then dropped).  Returns (advantages, returns)."""
    n = len(rewards)
    adv = np.zeros(n, np.float64)
    last = 0.0
    for t in reversed(range(n)):
        if t == n - 1:
            nonterminal, next_value = 1.0 - float(last_done), float(last_value)
        else:
            nonterminal, next_value = 1.0 - float(episode_starts[t + 1]), float(values[t + 1])
        delta = float(rewards[t]) + gamma * next_value * nonterminal - float(values[t])
        last = delta + gamma * lam * nonterminal * last
        adv[t] = last
    return adv, adv + np.asarray(values, np.float64)


def ppo_loss(logp_new, logp_old, ent, values, adv, returns, clip, ent_coef, vf_coef):
    """(loss, approximate KL) of one minibatch: advantages normalised as (A - mean) / (std + 1e-8) with the unbiased std, the clipped policy loss,
    -mean entropy, the MSE value loss."""
    adv = (adv - adv.mean()) / (adv.std() + 1e-8) if adv.numel() > 1 else adv
    ratio = torch.exp(logp_new - logp_old)
    policy = -torch.min(ratio * adv, torch.clamp(ratio, 1 - clip, 1 + clip) * adv).mean()
    value = ((returns - values) ** 2).mean()
    loss = policy + ent_coef * (-ent.mean()) + vf_coef * value
    log_ratio = (logp_new - logp_old).detach()
    kl = float(((torch.exp(log_ratio) - 1) - log_ratio).mean())
    return loss, kl


# ------------------------------------------------------------------------------------------------ the repaired policy and one environment step
def lstm2(x_seq, lstm):
    """The last hidden state of a 2-layer nn.LSTM (torch's gate order i, f, g, o) over a sequence [T, B, d], from its weights, in float64."""
    h_in = x_seq.double()
    for layer in range(2):
        Wi, Wh = getattr(lstm, 'weight_ih_l%d' % layer).double(), getattr(lstm, 'weight_hh_l%d' % layer).double()
        bi, bh = getattr(lstm, 'bias_ih_l%d' % layer).double(), getattr(lstm, 'bias_hh_l%d' % layer).double()
        H = Wh.shape[1]
        h, c = torch.zeros(h_in.shape[1], H, dtype=torch.float64), torch.zeros(h_in.shape[1], H, dtype=torch.float64)
        outs = []
        for t in range(h_in.shape[0]):
            gates = h_in[t] @ Wi.t() + bi + h @ Wh.t() + bh
            i, f, g, o = gates[:, :H], gates[:, H:2 * H], gates[:, 2 * H:3 * H], gates[:, 3 * H:]
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        h_in = torch.stack(outs, 0)
    return h_in[-1]


def policy_query(user_emb, item_emb, lstm, dnn0, dnn2, user_id, profile):
    """The repaired policy for ONE observation: E_u = user_emb[user_id], E_i = the mean of item_emb over the profile's items, the length-2 sequence
    (E_u, E_i) through the LSTM, q = Linear(ReLU(Linear(h_last))).  Returns q [d] in float64."""
    eu = user_emb.double()[user_id]
    ei = item_emb.double()[torch.as_tensor(profile, dtype=torch.long)].mean(0)
    h = lstm2(torch.stack([eu, ei], 0)[:, None, :], lstm)[0]
    return torch.relu(h @ dnn0.weight.double().t() + dnn0.bias.double()) @ dnn2.weight.double().t() + dnn2.bias.double()


def env_step(action, n_keep, targets, rng_state):
    """One environment step's profile, with the literal numpy call of the attacks' step on the global numpy.random state `rng_state` (restored into the
    global generator first).  Returns (sorted item list, the numpy.random state afterwards)."""
    np.random.set_state(rng_state)
    action = np.asarray(action).copy()
    ones_indices = np.where(action == 1)[0]
    if len(ones_indices) > n_keep:
        keep_indices = np.random.choice(ones_indices, size=n_keep, replace=False)
        action = np.zeros_like(action)
        action[keep_indices] = 1
    state = np.zeros(len(action))
    state[np.where(action == 1)[0]] = 1
    state[targets] = 1
    return np.where(state == 1)[0], np.random.get_state()


def unpack(words, I):
    """[B, W] int32 -> [B, I] bool (numpy, independent of arlib_amd.unpack_bits)."""
    w = np.asarray(words.cpu().numpy()).view(np.uint32).astype(np.uint64)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint64)) & np.uint64(1)
    return torch.from_numpy(bits.reshape(w.shape[0], -1)[:, :I].astype(bool))


def policy_loss(pol, users, profiles, actions, logp_old, adv, returns, clip, ent_coef, vf_coef):
    """The PPO loss of one minibatch for the repaired PoisonRec policy `pol` (a float64 copy: its parameters are the leaves), every piece restated:
    the query per observation (policy_query), the head's log-probability and entropy from their formulas, the value tower as the dense
    Linear(F + I, 64) on the one-hot userId concatenated with the multi-hot profile.  actions [B, I] of 0/1.  Returns (loss, KL)."""
    E = pol.item_embedding.weight
    F, I = pol.user_embedding.weight.shape[0], E.shape[0]
    q = torch.stack([policy_query(pol.user_embedding.weight, E, pol.LSTM, pol.DNN[0], pol.DNN[2], int(u), p) for u, p in zip(users, profiles)], 0)
    p = torch.softmax(q @ E.t(), dim=1)
    sp = torch.log1p(torch.exp(p))
    logp = (actions.double() * p - sp).sum(1)
    ent = (sp - p / (1 + torch.exp(-p))).sum(1)
    x = torch.zeros(len(users), F + I, dtype=torch.float64)
    for b, (u, prof) in enumerate(zip(users, profiles)):
        x[b, int(u)] = 1
        x[b, F + torch.as_tensor(prof, dtype=torch.long)] = 1
    W = torch.cat([pol.vf_user, pol.vf_item], 0)
    h = torch.tanh(x @ W + pol.vf_bias)
    h = torch.tanh(h @ pol.vf_second.weight.t() + pol.vf_second.bias)
    values = (h @ pol.value_net.weight.t() + pol.value_net.bias)[:, 0]
    return ppo_loss(logp, logp_old, ent, values, adv, returns, clip, ent_coef, vf_coef)

"""CPU restatement of the PPO rollout around the networks (models/ppo/storage.py, models/ppo/algo/ppo.py:38-87): the four
compute_returns recurrences in fp32 (numpy float32 rounds after every operation, as torch's fp32 tensors do), the normalised
advantages, recurrent_generator's indexing, and the loss with closed-form gradients in float64.  The same formulas through
torch autograd (loss_torch) give the float64 check of the closed forms and, in float32, the yardstick of the GPU tests: how
far torch's own fp32 lands from float64."""
import functools

import numpy as np
import torch

GAMMA, LAMBDA = 0.99, 0.95
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)


# ---- compute_returns (storage.py:89-128) -----------------------------------------------------------------------------------
def compute_returns(rewards, value_preds, masks, bad_masks, next_value, use_gae, gamma, gae_lambda, proper):
    """fp32 arrays (T,N,1) / (T+1,N,1) / (N,1) -> (returns (T+1,N,1), value_preds after the call), bit for bit the reference's."""
    f = np.float32
    r, v, m, bm = (np.array(a, dtype=f) for a in (rewards, value_preds, masks, bad_masks))
    T = r.shape[0]
    ret = np.zeros_like(v)
    g, gl = f(gamma), f(gamma * gae_lambda)
    if use_gae:
        v[T] = next_value
        a = np.zeros_like(v[0])
        for t in reversed(range(T)):
            d = (r[t] + (g * v[t + 1]) * m[t + 1]) - v[t]
            a = d + (gl * m[t + 1]) * a
            if proper:
                a = a * bm[t + 1]
            ret[t] = a + v[t]
    else:
        ret[T] = next_value
        for t in reversed(range(T)):
            if proper:
                ret[t] = ((ret[t + 1] * g) * m[t + 1] + r[t]) * bm[t + 1] + (f(1) - bm[t + 1]) * v[t]
            else:
                ret[t] = (ret[t + 1] * g) * m[t + 1] + r[t]
    assert ret.dtype == f and v.dtype == f
    return ret, v


def advantages64(returns, value_preds):
    """ppo.py:39-41 in float64 on the fp32 difference returns[:-1] - value_preds[:-1] (the subtraction is the kernel's and
    torch's first fp32 operation; its result is the common input)."""
    a = (returns[:-1] - value_preds[:-1]).astype(np.float32).astype(np.float64)
    return (a - a.mean()) / (a.std(ddof=1) + 1e-5)


def advantages_torch32(returns, value_preds):
    a = torch.from_numpy(returns[:-1]) - torch.from_numpy(value_preds[:-1])
    return ((a - a.mean()) / (a.std() + 1e-5)).numpy()


def rollout_inputs(T, N, seed, zero_mask_rows=True):
    """Random fp32 storage contents; masks / bad_masks random in {0, 1}, with masks = 0 at the last and the first step."""
    r = np.random.default_rng(seed)
    f = np.float32
    d = dict(rewards=r.normal(size=(T, N, 1)).astype(f), value_preds=r.normal(size=(T + 1, N, 1)).astype(f),
             masks=(r.random((T + 1, N, 1)) < 0.8).astype(f), bad_masks=(r.random((T + 1, N, 1)) < 0.8).astype(f),
             next_value=r.normal(size=(N, 1)).astype(f))
    if zero_mask_rows:
        d["masks"][T, 0] = 0.0                                   # the step after the last one starts an episode
        d["masks"][1, N - 1] = 0.0                               # and so does the one after the first
        d["bad_masks"][T, N // 2] = 0.0
    return d


def advantage_error32(ret, v):
    """max |torch fp32 - float64| of the normalised advantages of these returns and value_preds."""
    return float(np.abs(advantages_torch32(ret, v) - advantages64(ret, v)).max())


@functools.lru_cache(maxsize=None)
def advantage_distance(T, N, use_gae=True, proper=True, seeds=20):
    """The largest advantage_error32 over `seeds` draws at this shape and mode.  A test adds the error on its own input: with
    few values the normalisation can be ill-conditioned (two nearly equal advantages), for torch as for anybody."""
    worst = 0.0
    for s in range(seeds):
        d = rollout_inputs(T, N, 1000 + s)
        worst = max(worst, advantage_error32(*compute_returns(d["rewards"], d["value_preds"], d["masks"], d["bad_masks"],
                                                               d["next_value"], use_gae, GAMMA, LAMBDA, proper)))
    return worst


# ---- recurrent_generator (storage.py:173-245) ------------------------------------------------------------------------------
def minibatches(stores, hidden, perm, num_mini_batch):
    """stores: {name: (T or T+1, N, ...)} (the first T steps are taken), hidden (T+1, N, H), perm: the env permutation.
    Row t * nb + j of a minibatch is step t of env perm[start + j]; the hidden state is slot 0 of those envs.  The last
    minibatch is short when num_mini_batch does not divide N."""
    N = hidden.shape[1]
    per = N // num_mini_batch
    T = min(a.shape[0] for a in stores.values())
    out = []
    for start in range(0, N, per):
        envs = np.asarray(perm[start:start + per])
        mb = {k: a[:T][:, envs].reshape(T * len(envs), *a.shape[2:]) for k, a in stores.items()}
        mb["recurrent_hidden_states"] = hidden[0][envs]
        out.append(mb)
    return out


# ---- the loss (ppo.py:66-87) -----------------------------------------------------------------------------------------------
def loss_ref(kind, head, logstd, value, action, old_logp, adv, returns, value_preds, clip, vcoef, ecoef, clipped):
    """float64 closed forms: {'out': [value_loss, action_loss, dist_entropy, total], 'g_head', 'g_value', 'g_logstd'}."""
    d = np.float64
    head, value, old_logp, adv, returns = (np.asarray(a, dtype=d) for a in (head, value, old_logp, adv, returns))
    M, n = head.shape
    v, rt, ol, ad = value.reshape(M), returns.reshape(M), old_logp.reshape(M), adv.reshape(M)
    if kind == 0:
        ls = np.asarray(logstd, dtype=d).reshape(n)
        diff, var = np.asarray(action, dtype=d) - head, np.exp(ls) ** 2
        logp = (-(diff ** 2) / (2 * var) - ls - HALF_LOG_2PI).sum(1)
        entropy = (0.5 + HALF_LOG_2PI + ls).mean()
    else:
        a = np.asarray(action).reshape(M)
        z = head - head.max(1, keepdims=True)
        lsm = z - np.log(np.exp(z).sum(1, keepdims=True))
        p = np.exp(lsm)
        logp = lsm[np.arange(M), a]
        H = -(p * lsm).sum(1)
        entropy = H.mean()
    ratio = np.exp(logp - ol)
    s1, s2 = ratio * ad, np.clip(ratio, 1 - clip, 1 + clip) * ad
    action_loss = -np.minimum(s1, s2).mean()
    glp = np.where(s1 <= s2, -ad * ratio / M, 0.0)
    if clipped:
        vp = np.asarray(value_preds, dtype=d).reshape(M)
        dv = v - vp
        vpc = vp + np.clip(dv, -clip, clip)
        l1, l2 = (v - rt) ** 2, (vpc - rt) ** 2
        value_loss = 0.5 * np.maximum(l1, l2).mean()
        w1 = np.where(l1 > l2, 1.0, np.where(l1 == l2, 0.5, 0.0))
        gate = (np.abs(dv) <= clip).astype(d)
        gv = (w1 * (v - rt) + (1 - w1) * gate * (vpc - rt)) / M
    else:
        value_loss = 0.5 * ((rt - v) ** 2).mean()
        gv = (v - rt) / M
    total = value_loss * vcoef + action_loss - entropy * ecoef
    res = {"out": np.array([value_loss, action_loss, entropy, total]), "g_value": (vcoef * gv).reshape(M, 1)}
    if kind == 0:
        res["g_head"] = glp[:, None] * diff / var
        res["g_logstd"] = (glp[:, None] * (diff ** 2 / var - 1)).sum(0) - ecoef / n
    else:
        onehot = np.zeros((M, n))
        onehot[np.arange(M), a] = 1.0
        res["g_head"] = glp[:, None] * (onehot - p) + (ecoef / M) * p * (lsm + H[:, None])
    return res


def loss_torch(kind, head, logstd, value, action, old_logp, adv, returns, value_preds, clip, vcoef, ecoef, clipped, dtype):
    """The reference's lines (distributions.py FixedNormal / FixedCategorical, model.py:79-80, ppo.py:66-87) through torch
    autograd on the CPU in `dtype`; same result dict as loss_ref (numpy, `dtype`)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)        # noqa: E731
    head_t, values = t(head).requires_grad_(), t(value).reshape(-1, 1).requires_grad_()
    M = head_t.shape[0]
    old, adv_t, ret, vp = (t(a).reshape(M, 1) for a in (old_logp, adv, returns, value_preds))
    if kind == 0:
        ls = t(logstd).reshape(-1, 1).requires_grad_()               # AddBias: _bias (n,1), added as _bias.t().view(1,-1)
        dist = torch.distributions.Normal(head_t, (torch.zeros_like(head_t) + ls.t().view(1, -1)).exp())
        action_log_probs = dist.log_prob(t(action)).sum(-1, keepdim=True)
    else:
        ls = None
        dist = torch.distributions.Categorical(logits=head_t)
        act = torch.from_numpy(np.ascontiguousarray(action)).reshape(M, 1)
        action_log_probs = dist.log_prob(act.squeeze(-1)).view(M, -1).sum(-1).unsqueeze(-1)
    dist_entropy = dist.entropy().mean()
    ratio = torch.exp(action_log_probs - old)
    surr1 = ratio * adv_t
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv_t
    action_loss = -torch.min(surr1, surr2).mean()
    if clipped:
        value_pred_clipped = vp + (values - vp).clamp(-clip, clip)
        value_losses = (values - ret).pow(2)
        value_losses_clipped = (value_pred_clipped - ret).pow(2)
        value_loss = 0.5 * torch.max(value_losses, value_losses_clipped).mean()
    else:
        value_loss = 0.5 * (ret - values).pow(2).mean()
    total = value_loss * vcoef + action_loss - dist_entropy * ecoef
    total.backward()
    res = {"out": torch.stack([value_loss, action_loss, dist_entropy, total]).detach().numpy(),
           "g_head": head_t.grad.numpy(), "g_value": values.grad.numpy()}
    if kind == 0:
        res["g_logstd"] = ls.grad.reshape(-1).numpy()
    return res


CLIP, VCOEF, ECOEF = 0.2, 0.5, 0.01


def loss_inputs(kind, M, n, seed, clip=CLIP):
    """fp32 inputs in which no row sits near a kink: a row is drawn again while its float64 ratio is within 1e-3 of
    1 +- clip, |v - vp| within 1e-3 of clip, or (v - ret)^2 within 1e-3 of (vpc - ret)^2."""
    r = np.random.default_rng(seed)
    f = np.float32

    def draw(m):
        d = {"head": r.normal(scale=1.0 if kind == 0 else 2.0, size=(m, n)).astype(f), "value": r.normal(size=(m, 1)).astype(f),
             "adv": r.normal(size=(m, 1)).astype(f), "returns": r.normal(size=(m, 1)).astype(f)}
        d["value_preds"] = (d["value"] + r.normal(scale=0.3, size=(m, 1))).astype(f)
        if kind == 0:
            d["action"] = (d["head"] + r.normal(scale=0.7, size=(m, n))).astype(f)
        else:
            d["action"] = r.integers(0, n, size=(m, 1)).astype(np.int64)
        d["old_shift"] = r.normal(scale=0.25, size=(m, 1)).astype(f)
        return d

    logstd = r.uniform(-1.0, 0.0, size=n).astype(f) if kind == 0 else None
    d = draw(M)

    def finish(d):
        logp = logp64(kind, d["head"], logstd, d["action"])
        d["old_logp"] = (logp[:, None] + d["old_shift"]).astype(f)
        ratio = np.exp(logp - d["old_logp"][:, 0].astype(np.float64))
        v, vp, rt = (d[k][:, 0].astype(np.float64) for k in ("value", "value_preds", "returns"))
        vpc = vp + np.clip(v - vp, -clip, clip)
        bad = (np.abs(ratio - (1 - clip)) < 1e-3) | (np.abs(ratio - (1 + clip)) < 1e-3)
        bad |= np.abs(np.abs(v - vp) - clip) < 1e-3
        bad |= np.abs((v - rt) ** 2 - (vpc - rt) ** 2) < 1e-3
        return bad

    bad = finish(d)
    while bad.any():
        fresh = draw(int(bad.sum()))
        for k in fresh:
            d[k][bad] = fresh[k]
        bad = finish(d)
    d.pop("old_shift")
    d["logstd"] = logstd
    return d


def logp64(kind, head, logstd, action):
    h = np.asarray(head, dtype=np.float64)
    if kind == 0:
        ls = np.asarray(logstd, dtype=np.float64)
        return (-((np.asarray(action, dtype=np.float64) - h) ** 2) / (2 * np.exp(ls) ** 2) - ls - HALF_LOG_2PI).sum(1)
    z = h - h.max(1, keepdims=True)
    lsm = z - np.log(np.exp(z).sum(1, keepdims=True))
    return lsm[np.arange(len(h)), np.asarray(action).reshape(-1)]


def loss_args(d, clipped, clip=CLIP):
    return (d["head"], d["logstd"], d["value"], d["action"], d["old_logp"], d["adv"], d["returns"], d["value_preds"], clip, VCOEF,
            ECOEF, clipped)


@functools.lru_cache(maxsize=None)
def loss_distance(kind, M, n, clipped, seeds=20):
    """Per output array, the largest over `seeds` draws of max |torch fp32 autograd - float64 closed form| / max |float64| at
    this case: fp32 rounding scales with the numbers it rounds, and a one-row gradient's size varies a lot from draw to draw,
    so the distance is taken relative to the array's largest magnitude (an all-zero array counts with its absolute error)."""
    worst = {}
    for s in range(seeds):
        d = loss_inputs(kind, M, n, 5000 + s)
        ref = loss_ref(kind, *loss_args(d, clipped))
        t32 = loss_torch(kind, *loss_args(d, clipped), dtype=torch.float32)
        for k in ref:
            err = float(np.abs(t32[k].astype(np.float64).reshape(ref[k].shape) - ref[k]).max())
            worst[k] = max(worst.get(k, 0.0), err / scale(ref[k]))
    return worst


def scale(a):
    m = float(np.abs(a).max())
    return m if m > 0 else 1.0

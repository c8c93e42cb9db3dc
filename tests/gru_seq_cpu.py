"""CPU restatement of the PPO update's recurrent sequence (models/ppo/model.py:116-171, NNBase._forward_gru), the checker of
csrc/gru_seq.hip / var_amd.masked_gru.

masked_gru_steps   THE definition (include/var_hip.h), step by step in any dtype, differentiable by torch autograd:
                       h' = h_{t-1} * m_t;  gi = W_ih x_t + b_ih;  gh = W_hh h' + b_hh
                       r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h_t = (1 - z) * n + z * h'
segmented_gru      the reference's form in this project's words: cut the sequence at every step t >= 1 where some mask is 0, run
                   torch.nn.GRU over each piece from (state * masks[first step of the piece]), concatenate.
For 0/1 masks the two are the same function: inside a piece every mask is 1.0 and h * 1.0 == h bit for bit.

Bounds (tests/rollout_cpu.py's rule): per output array, four times the distance of torch's own fp32 CPU evaluation of the
segmented form from the float64 definition -- the largest over 20 seeded draws at the tested shape, relative to the array's
largest magnitude (gru_distance).  The factor four covers a different summation order and the device's expf / tanhf; the
yardstick is torch against float64, never the kernel.  The gates are smooth: no row is left out of any comparison."""
import functools

import numpy as np
import torch
import torch.nn as nn

OUTPUTS = ("out", "h_T")
GRADS = ("d_x", "d_hxs", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")
PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
MARGIN = 4.0


def masked_gru_steps(x, hxs, masks, w_ih, w_hh, b_ih, b_hh):
    """torch tensors of one dtype: x (T*N, I), hxs (N, H), masks (T*N, 1) -> out (T*N, H), h_T (N, H)."""
    N, H = hxs.shape
    T = x.shape[0] // N
    xs, ms = x.view(T, N, -1), masks.view(T, N, 1)
    h, outs = hxs, []
    for t in range(T):
        hp = h * ms[t]
        gi = xs[t] @ w_ih.t() + b_ih
        gh = hp @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1 - z) * n + z * hp
        outs.append(h)
    return torch.cat(outs, 0), h


def segmented_gru(gru, x, hxs, masks):
    """The segmented form over an nn.GRU, host-side cuts (CPU tensors)."""
    N = hxs.shape[0]
    if x.shape[0] == N:
        out, h = gru(x.unsqueeze(0), (hxs * masks).unsqueeze(0))
        return out.squeeze(0), h.squeeze(0)
    T = x.shape[0] // N
    xs, ms = x.view(T, N, -1), masks.view(T, N)
    cuts = [0] + [t for t in range(1, T) if bool((ms[t] == 0.0).any())] + [T]
    h, outs = hxs.unsqueeze(0), []
    for a, b in zip(cuts[:-1], cuts[1:]):
        o, h = gru(xs[a:b], h * ms[a].view(1, -1, 1))
        outs.append(o)
    return torch.cat(outs, 0).view(T * N, -1), h.squeeze(0)


def gru_inputs(T, N, I, H, seed, orthogonal=False):
    """fp32 numpy inputs: non-zero hxs, small non-zero biases, 0/1 masks with zeros (one at t = 0 and one at the last step
    unless T * N = 1), d_out and d_hT.  Weights: nn.init.orthogonal_ (the reference's, model.py:96-100) or Gaussian
    rows of the scale of nn.GRU's own initialisation (cheap enough for 20 draws of a 3072 x 1024 matrix)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    if orthogonal:
        torch.manual_seed(seed)
        w_ih, w_hh = torch.empty(3 * H, I), torch.empty(3 * H, H)
        nn.init.orthogonal_(w_ih)
        nn.init.orthogonal_(w_hh)
    else:
        w_ih, w_hh = rn(3 * H, I) / float(I) ** 0.5, rn(3 * H, H) / float(H) ** 0.5
    masks = (torch.rand(T, N, generator=g) < 0.75).float()
    if T * N > 1:
        masks[0, 0] = 0.0
        masks[T - 1, N - 1] = 0.0
    else:
        masks[0, 0] = 1.0                                         # (the one state there is reaches the recurrent product)
    if N > 1:
        masks[0, 1] = 1.0
    d = {"x": rn(T * N, I), "hxs": rn(N, H) * 0.5, "masks": masks.view(T * N, 1), "w_ih": w_ih, "w_hh": w_hh,
         "b_ih": rn(3 * H) * 0.1, "b_hh": rn(3 * H) * 0.1, "d_out": rn(T * N, H), "d_hT": rn(N, H)}
    return {k: v.numpy().astype(np.float32) for k, v in d.items()}


def evaluate(d, dtype, form="steps", with_dhT=True, both=False):
    """Outputs and the six gradients of sum(out * d_out) (+ sum(h_T * d_hT)) as float64 numpy arrays, on the CPU in `dtype`.
    form: "steps" (the definition) or "segmented" (torch.nn.GRU per piece).  both: returns (without d_hT, with d_hT)."""
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dtype) for k, v in d.items()}
    if form == "steps":
        leaves = [t[k].requires_grad_() for k in ("x", "hxs") + PARAMS]
        out, h_T = masked_gru_steps(t["x"], t["hxs"], t["masks"], *(t[k] for k in PARAMS))
    else:
        gru = nn.GRU(t["w_ih"].shape[1], t["w_hh"].shape[1]).to(dtype)
        mine = (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
        with torch.no_grad():
            for prm, k in zip(mine, PARAMS):
                prm.copy_(t[k])
        leaves = [t["x"].requires_grad_(), t["hxs"].requires_grad_(), *mine]
        out, h_T = segmented_gru(gru, t["x"], t["hxs"], t["masks"])

    def result(with_h):
        obj = (out * t["d_out"]).sum()
        if with_h:
            obj = obj + (h_T * t["d_hT"]).sum()
        g = torch.autograd.grad(obj, leaves, retain_graph=True)
        res = {"out": out, "h_T": h_T}
        res.update(zip(GRADS, g))
        return {k: v.detach().double().numpy() for k, v in res.items()}

    if both:
        return result(False), result(True)
    return result(with_dhT)


def scale(a):
    m = float(np.abs(a).max())
    return m if m > 0 else 1.0


def rel(got, ref):
    """max |got - ref| / max |ref| (an all-zero reference counts with the absolute error)."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64).reshape(ref.shape) - ref).max()) / scale(ref)


@functools.lru_cache(maxsize=None)
def gru_distance(T, N, I, H, seeds=20):
    """{False: {...}, True: {...}} (without / with d_hT): per array, the largest over `seeds` draws of
    rel(torch fp32 segmented, float64 definition) at this shape."""
    worst = {False: {}, True: {}}
    for s in range(seeds):
        d = gru_inputs(T, N, I, H, 9000 + s)
        ref = evaluate(d, torch.float64, "steps", both=True)
        t32 = evaluate(d, torch.float32, "segmented", both=True)
        for w, r, a in zip((False, True), ref, t32):
            for k in r:
                worst[w][k] = max(worst[w].get(k, 0.0), rel(a[k], r[k]))
    return worst


def gru_bounds(T, N, I, H, with_dhT):
    return {k: MARGIN * v for k, v in gru_distance(T, N, I, H)[bool(with_dhT)].items()}


# ---- a stand-in recurrent actor-critic for PPO.loss: GRU + two Linear layers + DiagGaussian ----------------------------------------
class AddBias(nn.Module):
    def __init__(self, n):
        super().__init__()
        self._bias = nn.Parameter(torch.zeros(n, 1))

    def forward(self, x):
        return x + self._bias.t().view(1, -1)


class StandInDist(nn.Module):
    def __init__(self, H, n):
        super().__init__()
        self.fc_mean = nn.Linear(H, n)
        self.logstd = AddBias(n)


class StandInBase(nn.Module):
    def __init__(self, I, H):
        super().__init__()
        self.gru = nn.GRU(I, H)
        self.critic_linear = nn.Linear(H, 1)

    def _forward_gru(self, x, hxs, masks):
        return segmented_gru(self.gru, x, hxs, masks)

    def forward(self, inputs, rnn_hxs, masks, infer=False):
        x, rnn_hxs = self._forward_gru(inputs, rnn_hxs, masks)
        return self.critic_linear(x), x, rnn_hxs, None


class StandInPolicy(nn.Module):
    is_recurrent = True

    def __init__(self, I, H, n, seed):
        super().__init__()
        torch.manual_seed(seed)
        self.base = StandInBase(I, H)
        self.dist = StandInDist(H, n)
        with torch.no_grad():
            self.dist.logstd._bias.uniform_(-1.0, 0.0)


CLIP, VCOEF, ECOEF = 0.2, 0.5, 0.01


def ppo_total(policy, sample):
    """The loss lines of models/ppo/algo/ppo.py:55-87 (DiagGaussian, clipped value loss) in torch, in the policy's dtype."""
    obs, hxs, actions, value_preds, returns, masks, old_logp, adv = sample
    values, feats, _, _ = policy.base(obs, hxs, masks)
    mean = policy.dist.fc_mean(feats)
    dist = torch.distributions.Normal(mean, policy.dist.logstd(torch.zeros_like(mean)).exp())
    logp = dist.log_prob(actions).sum(-1, keepdim=True)
    entropy = dist.entropy().mean()                              # (FixedNormal's own sum is misspelt: Normal's runs)
    ratio = torch.exp(logp - old_logp)
    surr1, surr2 = ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    vpc = value_preds + (values - value_preds).clamp(-CLIP, CLIP)
    value_loss = 0.5 * torch.max((values - returns).pow(2), (vpc - returns).pow(2)).mean()
    return value_loss * VCOEF + action_loss - entropy * ECOEF


def ppo_sample(policy64, T, N, I, n, seed):
    """A minibatch (fp32 numpy, recurrent_generator's order) that keeps every row away from the loss's kinks: the old log
    probabilities put the ratio within [0.9, 1.1] of 1 and the old value predictions within 0.15 of the values (clip = 0.2)
    -- there both clamps are the identity in fp32 as in float64 -- and the returns at least 0.5 from the values."""
    r = np.random.default_rng(seed)
    H = policy64.base.gru.hidden_size
    f = np.float32
    masks = (r.random((T, N)) < 0.75).astype(f)
    masks[0, 0] = 0.0
    s = {"obs": r.normal(size=(T * N, I)).astype(f), "hxs": (0.5 * r.normal(size=(N, H))).astype(f),
         "masks": masks.reshape(T * N, 1), "adv": r.normal(size=(T * N, 1)).astype(f)}
    t64 = lambda a: torch.from_numpy(a).double()                  # noqa: E731
    with torch.no_grad():
        values, feats, _, _ = policy64.base(t64(s["obs"]), t64(s["hxs"]), t64(s["masks"]))
        mean = policy64.dist.fc_mean(feats)
        std = policy64.dist.logstd(torch.zeros_like(mean)).exp()
        actions = (mean + std * torch.from_numpy(r.normal(size=(T * N, n)))).numpy().astype(f)
        logp = torch.distributions.Normal(mean, std).log_prob(t64(actions)).sum(-1, keepdim=True).numpy()
    values = values.numpy()
    sign = lambda: np.where(r.random((T * N, 1)) < 0.5, -1.0, 1.0)  # noqa: E731
    s["actions"] = actions
    s["old_logp"] = (logp + sign() * r.uniform(0.01, 0.09, size=(T * N, 1))).astype(f)
    s["value_preds"] = (values + sign() * r.uniform(0.02, 0.15, size=(T * N, 1))).astype(f)
    s["returns"] = (values + sign() * r.uniform(0.5, 1.5, size=(T * N, 1))).astype(f)
    return s


def sample_tuple(s, to):
    return tuple(to(s[k]) for k in ("obs", "hxs", "actions", "value_preds", "returns", "masks", "old_logp", "adv"))


def ppo_param_grads(policy, s, dtype):
    pol = policy.to(dtype)
    pol.zero_grad()
    ppo_total(pol, sample_tuple(s, lambda a: torch.from_numpy(a).to(dtype))).backward()
    return {k: v.grad.detach().double().numpy().copy() for k, v in pol.named_parameters()}


@functools.lru_cache(maxsize=None)
def ppo_distance(T, N, I, H, n, seeds=20):
    """Per parameter of the stand-in, the largest over `seeds` draws of rel(torch fp32 CPU gradient, float64 gradient)."""
    import copy
    worst = {}
    for sd in range(seeds):
        p64 = StandInPolicy(I, H, n, 7000 + sd).double()
        s = ppo_sample(p64, T, N, I, n, 7100 + sd)
        g64 = ppo_param_grads(p64, s, torch.float64)
        g32 = ppo_param_grads(copy.deepcopy(p64), s, torch.float32)
        for k in g64:
            worst[k] = max(worst.get(k, 0.0), rel(g32[k], g64[k]))
    return worst


# ---- the fixture made from the reference (tests/golden/make_golden_gru_seq.py) ------------------------------------------------
FIXTURE_SHAPE = (7, 5, 128, 512)
ROWS = 16


@functools.lru_cache(maxsize=None)
def load_fixture(golden_dir):
    """(inputs as gru_inputs gives them, the whole main file): the weights come from their own files (1 MiB per file)."""
    import os
    g = dict(np.load(os.path.join(golden_dir, "gru_seq_t7.npz")))
    d = {k: g[k] for k in ("x", "hxs", "masks", "b_ih", "b_hh", "d_out", "d_hT")}
    d["w_ih"] = np.load(os.path.join(golden_dir, "gru_seq_t7_w_ih.npz"))["w_ih"]
    d["w_hh"] = np.concatenate([np.load(os.path.join(golden_dir, f"gru_seq_t7_w_hh{k}.npz"))["w_hh"] for k in range(4)])
    return d, g


def fixture_distances(got, g, with_dhT):
    """rel() of each array of `got` (out, h_T, the six gradients; numpy) from the fixture's; the two weight gradients through
    the rows and the sums the fixture keeps of them (the worst of the three)."""
    tag = "g1." if with_dhT else "g0."
    res = {}
    for k in OUTPUTS:
        if k in got:
            res[k] = rel(got[k], g[k])
    for k in GRADS:
        if k not in got:
            continue
        a = np.asarray(got[k], dtype=np.float64)
        if k in ("d_w_ih", "d_w_hh"):
            res[k] = max(rel(a[::ROWS], g[tag + k + ".rows16"]), rel(a.sum(1), g[tag + k + ".rowsum"]),
                         rel(a.sum(0), g[tag + k + ".colsum"]))
        else:
            res[k] = rel(a, g[tag + k])
    return res

"""CPU restatement of var_clip_adam_step (csrc/clip_adam.hip) -- torch.nn.utils.clip_grad_norm_ (norm type 2) followed by
torch.optim.Adam.step() over a list of tensors -- in float64, its seeded inputs, and the yardsticks of tests/test_gpu_clip_adam.py:
how far torch's own fp32 CPU evaluation of the whole composite, clip and then Adam, lands from float64 (the convention of
tests/step_tail_cpu.py, on which this file is built: the largest over 20 seeded draws at the tested shape, step and clip case, per
output).

Outputs and scales.  total_norm: relative.  m, v and the update u = p - p': step_tail_cpu's scales without cancellation, taken
at the clipped gradient g' = g * coef of the float64 composite (m: |m| + |g'|, v: v', u: S = (lr / bc1) (|m| + |g'|) / denom).  The
update is pinned by the form with p = 0, where p' is the negated update and nothing else; the general form asks
|p - p64| <= max(ulp32(p), ulp32(p64)) / 2 + 4 D_u S, as step_tail_cpu.adam_p_excess does.

Hyper-parameters are taken as the C floats the entry receives (step_tail_cpu's docstring says why), and so is the 1e-6 that
clip_grad_norm_ adds to the norm: fp32 torch adds float32(1e-6), and so does the kernel."""
import collections
import functools

import numpy as np
import torch

from tests import step_tail_cpu as st

SEEDS = st.SEEDS
CLIP_EPS = st.f32(1e-6)
# the reference's PPO values: RLLr, RLEps, RLMaxGradNorm of Envs/ai2thor/config.py:74-76 (= examples/config_commented.py:78-80),
# and optim.Adam's default betas (models/ppo/algo/ppo.py:32 passes none)
LR, EPS, MAX_NORM, BETAS = 6e-5, 1e-5, 0.5, (0.9, 0.999)
Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps max_norm step")      # max_norm None or <= 0: no clip


def hyper(step, max_norm=MAX_NORM, lr=LR):
    return Hyper(lr, BETAS[0], BETAS[1], EPS, max_norm, step)


def carried(h):
    mn = None if h.max_norm is None or h.max_norm <= 0 else st.f32(h.max_norm)
    return Hyper(st.f32(h.lr), st.f32(h.b1), st.f32(h.b2), st.f32(h.eps), mn, int(h.step))


def clip64(gs, max_norm, norm_eps=CLIP_EPS):
    """clip_grad_norm_ in float64 over a list of arrays: (total_norm, coef); max_norm None: (None, 1)."""
    if max_norm is None:
        return None, 1.0
    total = float(np.sqrt(sum(float(np.sum(np.square(np.asarray(g, np.float64)))) for g in gs)))
    return total, min(max_norm / (total + norm_eps), 1.0)


def clip_adam64(ps, gs, ms, vs, h, norm_eps=CLIP_EPS):
    """The composite in float64 at the hyper-parameters h AS GIVEN: (total_norm or None, coef, [(p', m', v', u)] per tensor)."""
    total, coef = clip64(gs, h.max_norm, norm_eps)
    out = [st.adam64(p, np.asarray(g, np.float64) * coef, m, v, h.step, h.lr, h.b1, h.b2, h.eps, 0.0) for p, g, m, v in zip(ps, gs, ms, vs)]
    return total, coef, out


def clip_adam_torch(ps, gs, ms, vs, h, dtype):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) on the CPU in `dtype`, state planted (h.step - 1 steps so far):
    (total_norm or None, [p'], [m'], [v']) as numpy."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)                     # noqa: E731  (np.array: a copy)
    P = [torch.nn.Parameter(t(p)) for p in ps]
    for x, g in zip(P, gs):
        x.grad = t(g)
    opt = torch.optim.Adam(P, lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, foreach=False)
    for x, m, v in zip(P, ms, vs):
        opt.state[x] = {"step": torch.tensor(float(h.step - 1)), "exp_avg": t(m), "exp_avg_sq": t(v)}
    total = None
    if h.max_norm is not None:
        total = torch.nn.utils.clip_grad_norm_(P, h.max_norm, foreach=False).detach().numpy().copy()
    opt.step()
    return (total, [x.detach().numpy() for x in P], [opt.state[x]["exp_avg"].numpy() for x in P],
            [opt.state[x]["exp_avg_sq"].numpy() for x in P])


def inputs(lens, seed, form, h, norm_ratio):
    """fp32 arrays over sum(lens) elements (split() cuts them into the table's tensors): g with log-uniform magnitudes over ten
    decades and random signs, scaled so that its norm is norm_ratio * max_norm (0.5 * norm_ratio without a clip); m like g and v
    the square of such a draw -- both zero at step 1.  form 'zero': p = 0; 'general': p ~ N(0, 0.1^2).  Element 0 of a table of
    four or more elements has g = m = v = 0: nothing to do there, p keeps its bits."""
    assert form in ("zero", "general")
    n = int(sum(lens))
    r = np.random.default_rng(seed)
    f = np.float32

    def logu():
        x = np.exp(r.random(n, dtype=f) * f(np.log(1e10)) + f(np.log(1e-9)))
        return np.where(r.random(n, dtype=f) < 0.5, -x, x)

    g, m = logu(), logu()
    v = logu() ** 2
    target = norm_ratio * (h.max_norm if h.max_norm is not None and h.max_norm > 0 else 0.5)
    k = target / float(np.sqrt(np.sum(np.square(g.astype(np.float64)))))
    g = (g * k).astype(f)
    m, v = ((m * k).astype(f), (v * k * k).astype(f)) if h.step > 1 else (np.zeros(n, f), np.zeros(n, f))
    p = np.zeros(n, f) if form == "zero" else r.normal(0.0, 0.1, n).astype(f)
    if n >= 4:
        g[0] = m[0] = v[0] = 0.0
    return {"p": p, "g": g, "m": m, "v": v, "form": form}


def split(a, lens):
    return np.split(a, np.cumsum(lens)[:-1])


def reference(inp, h):
    """float64 results over the concatenation at the carried hyper-parameters, with step_tail_cpu's scales at g' = g * coef."""
    c = carried(h)
    total, coef, (out,) = clip_adam64([inp["p"]], [inp["g"]], [inp["m"]], [inp["v"]], c)
    p1, m1, v1, u = out
    g1 = inp["g"].astype(np.float64) * coef
    denom = np.sqrt(v1) / np.sqrt(1 - c.b2 ** c.step) + c.eps
    sm = np.abs(inp["m"].astype(np.float64)) + np.abs(g1)
    return {"tn": total, "coef": coef, "p": p1, "m": m1, "v": v1, "u": u, "sm": sm, "S": (c.lr / (1 - c.b1 ** c.step)) * sm / denom,
            "ok": np.ones(p1.shape, bool)}


def distances(inp, h, got_tn, got_p, got_m, got_v, ref=None):
    """{'tn' (with a clip), 'm', 'v'} and, for the p = 0 form, {'u'}: the distance of a result from float64, elementwise by the
    scales of reference() (the largest ratio), total_norm relatively.  A NaN is infinitely far."""
    ref = reference(inp, h) if ref is None else ref
    d = {"m": st._worst_ratio(np.abs(np.asarray(got_m, np.float64) - ref["m"]), ref["sm"], ref["ok"]),
         "v": st._worst_ratio(np.abs(np.asarray(got_v, np.float64) - ref["v"]), ref["v"], ref["ok"])}
    if ref["tn"] is not None:
        d["tn"] = abs(float(np.asarray(got_tn).reshape(-1)[0]) - ref["tn"]) / ref["tn"]
    if inp["form"] == "zero":
        d["u"] = st._worst_ratio(np.abs(-np.asarray(got_p, np.float64) - ref["u"]), ref["S"], ref["ok"])
    return {k: (np.inf if np.isnan(x) else x) for k, x in d.items()}


def p_excess(inp, h, got_p, d_u, ref=None, where=None):
    """The general form: max of |p_got - p64| / (max(ulp32(p), ulp32(p64)) / 2 + 4 d_u S), over the elements `where` (a slice)."""
    ref = reference(inp, h) if ref is None else ref
    w = slice(None) if where is None else where
    bound = 0.5 * np.maximum(st.ulp32(inp["p"][w]), st.ulp32(ref["p"][w])) + 4.0 * d_u * ref["S"][w]
    x = st._worst_ratio(np.abs(np.asarray(got_p, np.float64)[w] - ref["p"][w]), bound, ref["ok"][w])
    return np.inf if np.isnan(x) else x


@functools.lru_cache(maxsize=None)
def distance(lens, h, form, norm_ratio):
    """torch fp32's own distances() for the composite over a table of tensors of these lengths (a tuple), the largest over SEEDS
    draws at these hyper-parameters, this form and this clip case."""
    c = carried(h)
    worst = {}
    for s in range(SEEDS):
        inp = inputs(lens, 5000 + s, form, h, norm_ratio)
        tn, p, m, v = clip_adam_torch(*(split(inp[k], lens) for k in "pgmv"), c, torch.float32)
        for k, x in distances(inp, h, tn, np.concatenate(p), np.concatenate(m), np.concatenate(v)).items():
            worst[k] = max(worst.get(k, 0.0), x)
    return worst


def update_distance(lens, h, norm_ratio):
    """The update's fp32 distance at this case: from the p = 0 form, where p' is the update alone."""
    return distance(lens, h, "zero", norm_ratio)["u"]

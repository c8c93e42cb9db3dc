"""CPU restatement of the pretext step's tail -- the Adam step (csrc/pack_adam.hip), the triplet loss (csrc/heads.hip:
triplet_kernel) and the in-batch head (csrc/inbatch.hip) -- in float64, their seeded inputs, and the yardsticks of
tests/test_gpu_step_tail.py: how far torch's own fp32 CPU evaluation of the same formulas lands from float64 (the convention of
rollout_cpu.loss_distance: the largest over 20 seeded draws at the tested shape and hyper-parameters, per output array).

Hyper-parameters.  The C ABI carries every hyper-parameter as a C float, so the operation an entry can compute is the one with
float32(0.999), not with the decimal 0.999 (1 - float32(0.999) is 1.3e-5 away from 0.001, relatively: fifty times the fp32
rounding of exp_avg_sq).  Every reference here -- float64 and torch fp32 alike -- is therefore evaluated at carried(h), the
values the entry receives widened back to double, and the same holds for margin, tau, inv_count and the 1e-6 that
pairwise_distance adds (PD_EPS: fp32 torch adds float32(1e-6))."""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle.torch_oracle import inbatch_contrastive_loss

SEEDS = 20


def f32(x):
    """The value a C float argument carries, as a Python double."""
    return float(np.float32(x))


PD_EPS = f32(1e-6)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def scale(a):
    m = float(np.abs(a).max())
    return m if m > 0 else 1.0


# ---- Adam -------------------------------------------------------------------------------------------------------------------
Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd step")

HYPERS = (Hyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 1), Hyper(1e-4, 0.9, 0.999, 1e-8, 1e-6, 3), Hyper(1e-3, 0.9, 0.999, 1e-5, 0.1, 1000),
          Hyper(1e-4, 0.5, 0.9, 1e-3, 0.0, 7), Hyper(1e-4, 0.9, 0.999, 1e-8, 0.0, 100000))


def carried(h):
    return Hyper(f32(h.lr), f32(h.b1), f32(h.b2), f32(h.eps), f32(h.wd), int(h.step))


def adam64(p, g, m, v, step, lr, b1, b2, eps, wd):
    """torch's single-tensor Adam (torch/optim/adam.py: _single_tensor_adam, not capturable, no amsgrad) in float64.
    Returns p', m', v' and the update u = p - p'."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    g1 = g + wd * p
    m1 = m + (g1 - m) * (1 - b1)
    v1 = b2 * v + (1 - b2) * g1 * g1
    denom = np.sqrt(v1) / np.sqrt(1 - b2 ** step) + eps
    p1 = p - (lr / (1 - b1 ** step)) * m1 / denom
    return p1, m1, v1, p - p1


def adam_torch(p, g, m, v, step, lr, b1, b2, eps, wd, dtype):
    """torch.optim.Adam(foreach=False) on the CPU in `dtype` with its state planted (step - 1 steps taken so far)."""
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)                     # noqa: E731  (np.array: a copy)
    P = torch.nn.Parameter(t(p))
    P.grad = t(g)
    opt = torch.optim.Adam([P], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    opt.state[P] = {"step": torch.tensor(float(step - 1)), "exp_avg": t(m), "exp_avg_sq": t(v)}
    opt.step()
    st = opt.state[P]
    assert float(st["step"]) == step
    return P.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def adam_inputs(n, seed, form, wd=0.0):
    """fp32 (p, g, m, v) and the planted elements {'zero', 'eps', 'nan', 'cancel': index} (n >= 4; none below).
    g, m: log-uniform magnitudes in 1e-9 .. 10, random sign; v: the square of such a draw.  form 'zero': p = 0 (p' is then the
    negated update and nothing else); 'general': p ~ N(0, 0.1^2), and a gradient that would cancel against wd * p to less than
    half of |g| + |wd p| has its sign turned -- the scales below are free of cancellation only then."""
    assert form in ("zero", "general")
    r = np.random.default_rng(seed)
    f = np.float32

    def logu():
        x = np.exp(r.random(n, dtype=f) * f(np.log(1e10)) + f(np.log(1e-9)))
        return np.where(r.random(n, dtype=f) < 0.5, -x, x)

    g, m = logu(), logu()
    v = logu() ** 2
    p = np.zeros(n, f) if form == "zero" else r.normal(0.0, 0.1, n).astype(f)
    planted = {}
    if n >= 4:
        planted = {"zero": 0, "eps": n // 3, "nan": n // 2, "cancel": n - 1}
        i = planted["zero"]
        g[i] = m[i] = v[i] = 0.0                                  # nothing to do: with wd = 0, p keeps its bits
        g[planted["eps"]] = 1e-8                                   # |g| the size of eps
        g[planted["cancel"]] = f(-9.0) * m[planted["cancel"]]     # m' = m + (g - m) / 10 cancels at beta1 = 0.9
        g[planted["nan"]] = np.nan
    if form == "general" and wd != 0.0:
        w = f32(wd) * p.astype(np.float64)
        near = np.abs(g + w) < 0.5 * (np.abs(g) + np.abs(w))
        near[list(planted.values())] = False
        g[near] = -g[near]
    return {"p": p, "g": g, "m": m, "v": v, "planted": planted, "form": form}


def adam_ref(inp, h):
    """float64 results at the carried hyper-parameters, the cancellation-free scales, and the elements that count
    (all but the planted NaN): m by |m| + |g'|, v by v', the update by S = (lr / bc1) (|m| + |g'|) / denom."""
    c = carried(h)
    p, g, m, v = (inp[k].astype(np.float64) for k in "pgmv")
    p1, m1, v1, u = adam64(p, g, m, v, c.step, c.lr, c.b1, c.b2, c.eps, c.wd)
    g1 = g + c.wd * p
    denom = np.sqrt(v1) / np.sqrt(1 - c.b2 ** c.step) + c.eps
    sm = np.abs(m) + np.abs(g1)
    return {"p": p1, "m": m1, "v": v1, "u": u, "sm": sm, "S": (c.lr / (1 - c.b1 ** c.step)) * sm / denom, "ok": ~np.isnan(g)}


def _worst_ratio(err, sc, ok):
    """max over the counted elements of err / scale; where the scale is 0 the error has to be 0."""
    err, sc = err[ok], sc[ok]
    if err.size == 0:
        return 0.0
    q = np.where(sc > 0, err / np.where(sc > 0, sc, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(q.max())


def adam_distances(inp, h, got_p, got_m, got_v):
    """{'m', 'v'} and, for the p = 0 form, {'u'}: the largest elementwise distance of a result from float64 by the scales of
    adam_ref.  A NaN among the counted elements is infinitely far."""
    ref = adam_ref(inp, h)
    d = {"m": _worst_ratio(np.abs(np.asarray(got_m, np.float64) - ref["m"]), ref["sm"], ref["ok"]),
         "v": _worst_ratio(np.abs(np.asarray(got_v, np.float64) - ref["v"]), ref["v"], ref["ok"])}
    if inp["form"] == "zero":
        d["u"] = _worst_ratio(np.abs(-np.asarray(got_p, np.float64) - ref["u"]), ref["S"], ref["ok"])
    return {k: (np.inf if np.isnan(x) else x) for k, x in d.items()}


def adam_p_excess(inp, h, got_p, d_u):
    """The general form: max of |p_got - p64| / (max(ulp32(p), ulp32(p64)) / 2 + 4 d_u S) -- at most 1 when the parameter is
    the rounded float64 one up to four times the update's own fp32 distance."""
    ref = adam_ref(inp, h)
    bound = 0.5 * np.maximum(ulp32(inp["p"]), ulp32(ref["p"])) + 4.0 * d_u * ref["S"]
    x = _worst_ratio(np.abs(np.asarray(got_p, np.float64) - ref["p"]), bound, ref["ok"])
    return np.inf if np.isnan(x) else x


@functools.lru_cache(maxsize=None)
def adam_distance(n, h, form):
    """torch fp32 Adam's own adam_distances, the largest over SEEDS draws at this size, these hyper-parameters and this form."""
    c = carried(h)
    worst = {}
    for s in range(SEEDS):
        inp = adam_inputs(n, 1000 + s, form, h.wd)
        got = adam_torch(inp["p"], inp["g"], inp["m"], inp["v"], c.step, c.lr, c.b1, c.b2, c.eps, c.wd, torch.float32)
        for k, x in adam_distances(inp, h, *got).items():
            worst[k] = max(worst.get(k, 0.0), x)
    return worst


def adam_update_distance(n, h):
    """The update's fp32 distance at these hyper-parameters: from the p = 0, wd = 0 form, where p' is the update alone."""
    return adam_distance(n, h._replace(wd=0.0), "zero")["u"]


def graph_walk(table, cursor, ahead):
    """The row fetch and the cursor of one var_adam_step_graph launch (tests/_oracle_ctx.py): (index_row, new cursor)."""
    rows = table.shape[0]
    nxt = (int(cursor) + 1) % rows
    row = table[nxt] if not ahead else np.concatenate([table[nxt], table[(nxt + 1) % rows]])
    return row.copy(), nxt


# ---- triplet loss -----------------------------------------------------------------------------------------------------------
ACTIVE, INACTIVE, ZERO_DIST = 0, 1, 2


def triplet_inputs(B, seed, margin, mag=1.0):
    """fp32 (a, p, n) of magnitude `mag` and the kind of every row: two active rows (hinge argument >= margin / 20), then an
    inactive one (the negative farther than the positive by 1.5 margin and more), and so on; row B // 2 (B >= 2) has a = 0,
    p = float32(1e-6) -- (a - p) + float32(1e-6) is exactly 0 in fp32 -- and a negative within the margin."""
    r = np.random.default_rng(seed)
    unit = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)             # noqa: E731
    a, p, n = (mag * unit(r.standard_normal((B, 3))) for _ in range(3))
    kind = np.where(np.arange(B) % 3 == 2, INACTIVE, ACTIVE)
    ina = kind == INACTIVE
    p[ina] = a[ina] + 0.05 * mag * unit(r.standard_normal((int(ina.sum()), 3)))
    n[ina] = a[ina] + (0.05 * mag + margin * 1.5 + mag * r.random((int(ina.sum()), 1))) * unit(r.standard_normal((int(ina.sum()), 3)))
    a, p, n = (x.astype(np.float32) for x in (a, p, n))
    d = lambda x, y: np.linalg.norm(x.astype(np.float64) - y + PD_EPS, axis=1)  # noqa: E731
    swap = (kind == ACTIVE) & (d(a, p) - d(a, n) + margin < 0.05 * margin)
    p[swap], n[swap] = n[swap].copy(), p[swap].copy()
    if B >= 2:
        z = B // 2
        kind[z] = ZERO_DIST
        a[z], p[z] = 0.0, np.float32(1e-6)
        n[z] = (0.25 * margin * unit(r.standard_normal((1, 3)))).astype(np.float32)
    l = d(a, p) - d(a, n) + margin
    assert (l[kind != INACTIVE] >= 0.04 * margin).all() and (l[kind == INACTIVE] <= -0.4 * margin).all()
    return a, p, n, kind


def triplet_torch(a, p, n, margin, inv_count, dtype):
    """pairwise_distance(eps = PD_EPS) and clamp_min(d_ap - d_an + margin, 0), summed, times inv_count, through torch autograd
    on the CPU in `dtype`: {'loss', 'ga', 'gp', 'gn'} (numpy)."""
    ta, tp, tn = (torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_() for x in (a, p, n))
    l = torch.clamp_min(F.pairwise_distance(ta, tp, p=2, eps=PD_EPS) - F.pairwise_distance(ta, tn, p=2, eps=PD_EPS) + margin, 0)
    loss = l.sum() * inv_count
    loss.backward()
    return {"loss": loss.detach().numpy().reshape(1), "ga": ta.grad.numpy(), "gp": tp.grad.numpy(), "gn": tn.grad.numpy()}


def triplet64(a, p, n, margin, inv_count):
    return triplet_torch(a, p, n, margin, inv_count, torch.float64)


def _head_distance(ref, t32):
    return {k: float(np.abs(t32[k].astype(np.float64) - ref[k]).max()) / scale(ref[k]) for k in ref}


@functools.lru_cache(maxsize=None)
def triplet_distance(B, margin, inv_count, mag):
    """Per output, the largest over SEEDS draws of max |torch fp32 - float64| / max |float64| at this case."""
    worst = {}
    for s in range(SEEDS):
        a, p, n, _ = triplet_inputs(B, 3000 + s, margin, mag)
        for k, x in _head_distance(triplet64(a, p, n, f32(margin), f32(inv_count)),
                                   triplet_torch(a, p, n, f32(margin), f32(inv_count), torch.float32)).items():
            worst[k] = max(worst.get(k, 0.0), x)
    return worst


# ---- in-batch head ----------------------------------------------------------------------------------------------------------
def inbatch_inputs(B, M, seed):
    """Unit fp32 anchors (B,3) and candidates (M,3), int32 targets in [0, M): anchor 0 -> column 0, anchor 1 -> column M - 1,
    anchors 2 and 3 share a column, and the last anchor (B >= 2) is bit-equal to its positive: its distance is
    |(1e-6,1e-6,1e-6)|.  (A lone anchor on its positive has a loss of exp(-d/tau)'s size, which fp32 log-softmax cannot resolve
    from log(1 + x): torch's own fp32 is 100 % away from float64 there, and a yardstick of that size would pin nothing.)"""
    r = np.random.default_rng(seed)
    unit = lambda x: (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)      # noqa: E731
    a, cand = unit(r.standard_normal((B, 3))), unit(r.standard_normal((M, 3)))
    t = r.integers(0, M, B).astype(np.int32)
    t[0] = 0
    if B >= 2:
        t[1] = M - 1
    if B >= 4:
        t[3] = t[2]
    if B >= 2:
        a[B - 1] = cand[t[B - 1]]
    assert t.min() >= 0 and t.max() < M
    return a, cand, t


def inbatch_torch(a, cand, target, tau, inv_count, dtype):
    """oracle.torch_oracle.inbatch_contrastive_loss through torch autograd on the CPU in `dtype`: {'loss', 'ga', 'gc'}."""
    ta, tc = (torch.from_numpy(np.ascontiguousarray(x)).to(dtype).requires_grad_() for x in (a, cand))
    loss = inbatch_contrastive_loss(ta, tc, torch.from_numpy(np.asarray(target)).long(), tau=tau, inv_count=inv_count)
    loss.backward()
    return {"loss": loss.detach().numpy().reshape(1), "ga": ta.grad.numpy(), "gc": tc.grad.numpy()}


def inbatch64(a, cand, target, tau, inv_count):
    return inbatch_torch(a, cand, target, tau, inv_count, torch.float64)


@functools.lru_cache(maxsize=None)
def inbatch_distance(B, M, tau, inv_count):
    worst = {}
    for s in range(SEEDS):
        a, cand, t = inbatch_inputs(B, M, 7000 + s)
        for k, x in _head_distance(inbatch64(a, cand, t, f32(tau), f32(inv_count)),
                                   inbatch_torch(a, cand, t, f32(tau), f32(inv_count), torch.float32)).items():
            worst[k] = max(worst.get(k, 0.0), x)
    return worst

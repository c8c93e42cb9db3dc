"""CPU restatement of var_ppo_head_linear (include/var_hip.h): the distribution head's Linear (128 -> n), rollout_cpu's loss
on its result, and the five gradients, in float64.  The same chain through torch in float32 (F.linear, rollout_cpu.loss_torch,
autograd back through the Linear) is the yardstick of the GPU tests: per output array, how far torch's own fp32 lands from
float64, the largest over 20 seeded draws at the tested case; a test allows four times that (the project's standing margin).
Scales: an error counts relative to the array's largest magnitude, as in rollout_cpu.loss_distance -- except g_W and g_b, sums
over the rows whose terms cancel: fp32 rounding there grows with the sum of the terms' magnitudes, not with what is left of
them, so theirs is the largest such sum (clip_adam_cpu's "scales without cancellation"); relative to the remainder, the
yardstick's own error varies tenfold from draw to draw and no 20 draws bound the 21st."""
import functools

import numpy as np
import torch

from tests import rollout_cpu as rc

F = 128                                                          # actor features (both policies' hidden size)
ARRAYS = ("head", "out", "g_features", "g_W", "g_b", "g_value", "g_logstd")
KINK = 1e-3                                                      # rollout_cpu.loss_inputs' distance from a kink
FAULTS = {"no_bias": "head", "w_transposed": "g_features", "g_b_from_g_value": "g_b", "g_w_row_left_out": "g_W"}


def head64(features, W, b):
    return np.asarray(features, np.float64) @ np.asarray(W, np.float64).T + np.asarray(b, np.float64)


def ref(kind, d, clipped, clip=rc.CLIP):
    """float64: {'head', 'out', 'g_features', 'g_W', 'g_b', 'g_value', 'g_logstd' (kind 0)} of the inputs dict d, and under
    'scales' what errors() divides each array's error by."""
    head = head64(d["features"], d["W"], d["b"])
    res = rc.loss_ref(kind, head, d["logstd"], d["value"], d["action"], d["old_logp"], d["adv"], d["returns"], d["value_preds"], clip,
                      rc.VCOEF, rc.ECOEF, clipped)
    g_head = res.pop("g_head")
    res.update(head=head, g_features=g_head @ d["W"].astype(np.float64), g_W=g_head.T @ d["features"].astype(np.float64),
               g_b=g_head.sum(0))
    scales = {k: rc.scale(v) for k, v in res.items()}
    scales["g_W"] = rc.scale(np.abs(g_head).T @ np.abs(d["features"]).astype(np.float64))
    scales["g_b"] = rc.scale(np.abs(g_head).sum(0))
    res["scales"] = scales
    return res


def torch32(kind, d, clipped, clip=rc.CLIP, fault=None):
    """The same through torch in float32: F.linear, the reference's loss lines (rollout_cpu.loss_torch), autograd back through
    the Linear.  fault: one of FAULTS -- that array alone is computed wrongly, the others from the right values."""
    f = torch.from_numpy(d["features"]).requires_grad_()
    W, b = torch.from_numpy(d["W"]).requires_grad_(), torch.from_numpy(d["b"]).requires_grad_()
    head = torch.nn.functional.linear(f, W, b)
    res = rc.loss_torch(kind, head.detach().numpy(), d["logstd"], d["value"], d["action"], d["old_logp"], d["adv"], d["returns"],
                        d["value_preds"], clip, rc.VCOEF, rc.ECOEF, clipped, dtype=torch.float32)
    g_head = torch.from_numpy(res.pop("g_head"))
    head.backward(g_head)
    res.update(head=head.detach().numpy(), g_features=f.grad.numpy(), g_W=W.grad.numpy(), g_b=b.grad.numpy())
    if fault == "no_bias":
        res["head"] = torch.nn.functional.linear(f.detach(), W.detach()).numpy()
    elif fault == "w_transposed":
        res["g_features"] = (g_head @ W.detach().t().reshape(W.shape)).numpy()
    elif fault == "g_b_from_g_value":
        res["g_b"] = np.full_like(res["g_b"], res["g_value"].sum())
    elif fault == "g_w_row_left_out":
        res["g_W"] = (g_head[1:].t() @ f.detach()[1:]).numpy()
    elif fault is not None:
        raise ValueError(fault)
    return res


def near_kink(kind, d, clip=rc.CLIP, margin=KINK):
    """Per row, in float64: the ratio within `margin` of 1 +- clip, |v - vp| within it of clip, or -- outside the clip range,
    where they are two different numbers -- the two value losses within it of each other: where fp32 rounding may pick the
    other branch than float64.  (Inside the clip range vpc is v and both branches carry the same gradient.)"""
    logp = rc.logp64(kind, head64(d["features"], d["W"], d["b"]), d["logstd"], d["action"])
    ratio = np.exp(logp - d["old_logp"][:, 0].astype(np.float64))
    v, vp, rt = (d[k][:, 0].astype(np.float64) for k in ("value", "value_preds", "returns"))
    vpc = vp + np.clip(v - vp, -clip, clip)
    bad = (np.abs(ratio - (1 - clip)) < margin) | (np.abs(ratio - (1 + clip)) < margin)
    bad |= np.abs(np.abs(v - vp) - clip) < margin
    bad |= (np.abs(v - vp) > clip) & (np.abs((v - rt) ** 2 - (vpc - rt) ** 2) < margin)
    return bad


def inputs(kind, M, n, seed, clip=rc.CLIP):
    """fp32 inputs with no row near a kink (near_kink), and how many rows were drawn again to get there.  The weights have
    nn.Linear's scale, so the head has rollout_cpu.loss_inputs' spread."""
    r = np.random.default_rng(seed)
    f = np.float32
    W = (r.normal(size=(n, F)) * ((1.0 if kind == 0 else 2.0) / np.sqrt(F))).astype(f)
    b = r.normal(scale=0.1, size=n).astype(f)
    logstd = r.uniform(-1.0, 0.0, size=n).astype(f) if kind == 0 else None

    def draw(m):
        d = {"features": r.standard_normal((m, F), dtype=f), "value": r.normal(size=(m, 1)).astype(f),
             "adv": r.normal(size=(m, 1)).astype(f), "returns": r.normal(size=(m, 1)).astype(f)}
        d["value_preds"] = (d["value"] + r.normal(scale=0.3, size=(m, 1))).astype(f)
        head = head64(d["features"], W, b)
        if kind == 0:
            d["action"] = (head + r.normal(scale=0.7, size=(m, n))).astype(f)
        else:
            d["action"] = r.integers(0, n, size=(m, 1)).astype(np.int64)
        logp = rc.logp64(kind, head, logstd, d["action"])
        d["old_logp"] = (logp[:, None] + r.normal(scale=0.25, size=(m, 1))).astype(f)
        return d

    d = draw(M)
    d.update(W=W, b=b, logstd=logstd)
    redrawn = 0
    bad = near_kink(kind, d, clip)
    while bad.any():
        fresh = draw(int(bad.sum()))
        redrawn += int(bad.sum())
        for k in fresh:
            d[k][bad] = fresh[k]
        bad = near_kink(kind, d, clip)
    return d, redrawn


def errors(got, want):
    """Per array of `want` (a ref()): max |got - want| / its scale."""
    return {k: float(np.abs(np.asarray(got[k], np.float64).reshape(want[k].shape) - want[k]).max()) / want["scales"][k]
            for k in want if k != "scales"}


@functools.lru_cache(maxsize=None)
def distance(kind, M, n, clipped, seeds=20):
    """Per array, the largest error of torch32 against ref over `seeds` draws at this case."""
    worst = {}
    for s in range(seeds):
        d, _ = inputs(kind, M, n, 7000 + s)
        for k, e in errors(torch32(kind, d, clipped), ref(kind, d, clipped)).items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


def bounds(kind, M, n, clipped):
    """Four times distance(): what a test allows per array."""
    return {k: 4.0 * v for k, v in distance(kind, M, n, clipped).items()}

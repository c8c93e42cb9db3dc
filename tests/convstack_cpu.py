"""CPU restatement of the actor-critics' convolution stacks (include/var_hip.h, "The actor-critics' convolution stacks"), the
checker of csrc/convstack.hip / var_amd.conv_stack_eval: armNet_VAR.imgCNN's 96 x 96 branch (kind 0), ai2thorNet_VAR.imgCNN
(kind 1) and occupancyCNNMLP's two convolutions (kind 2), in torch, in either dtype, differentiable by torch autograd, over a dict
of parameters named as the Sequential's state_dict names them ('0.weight', '0.bias', '2.weight', ...).

Gates and choices (the device of tests/trunk_cpu.py).  A ReLU's gradient jumps where a pre-activation crosses zero between two
precisions, and a max pool's where two cells of a window swap rank.  The restatement therefore takes optional gate patterns and
pool choices: with them a ReLU is z * gate and a pool takes the chosen cell of each window, a function without kinks.  The
float64 backward a kernel is compared with is taken AT THE KERNEL'S OWN gates and choices; separately, every unit whose gate or
choice differs from the float64 forward's must be a near tie (flipped_units), and there may be at most trunk_cpu.MAX_FLIPS of
them.  A case's seed is the first at which torch's fp32 CPU evaluation shows none against float64 (find_seed).

Bounds: per output, saved activation and gradient array, four times the distance of torch's own fp32 CPU evaluation from float64
-- the largest over `draws` seeded draws at the tested shape, relative to the array's largest magnitude (convstack_distance);
five times against the fixtures made from the reference.  The yardstick is torch against float64, never the kernel."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from tests.gru_seq_cpu import rel, scale  # noqa: F401
from tests.trunk_cpu import FIXTURE_MARGIN, MARGIN, MAX_FLIPS, check_values  # noqa: F401

# per kind: input (C, H, W), then per convolution (in, out, stride, padding, a MaxPool2d(2, 2) follows)
STACKS = {
    0: ((3, 96, 96), ((3, 32, 1, 1, False), (32, 32, 1, 1, True), (32, 64, 1, 1, False), (64, 64, 1, 1, True), (64, 128, 1, 1, False),
                      (128, 128, 1, 1, True), (128, 256, 2, 0, False), (256, 128, 1, 0, False))),
    1: ((3, 96, 96), ((3, 32, 1, 1, False), (32, 32, 1, 1, True), (32, 64, 1, 1, True), (64, 64, 1, 1, True), (64, 128, 1, 1, True),
                      (128, 128, 2, 1, False))),
    2: ((1, 9, 9), ((1, 64, 2, 1, False), (64, 32, 2, 1, False))),
}


@functools.lru_cache(maxsize=None)
def layer_names(kind):
    """The convolutions' module indices in their Sequential, as strings ('0', '2', '5', ...)."""
    names, i = [], 0
    for *_rest, pooled in STACKS[kind][1]:
        names.append(str(i))
        i += 3 if pooled else 2
    return tuple(names)


def param_names(kind):
    return [f"{n}.{w}" for n in layer_names(kind) for w in ("weight", "bias")]


def feat_width(kind):
    return STACKS[kind][1][-1][1] * 9


def map_shapes(kind, B):
    """layer name -> (B, C, H, H) of its un-pooled post-ReLU map."""
    (_, h, _), convs = STACKS[kind]
    out = {}
    for name, (_cin, cout, stride, pad, pooled) in zip(layer_names(kind), convs):
        h = (h + 2 * pad - 3) // stride + 1
        out[name] = (B, cout, h, h)
        h = h // 2 if pooled else h
    return out


def convstack_params(kind, seed):
    """Seeded fp32 Gaussian weights of the scale of a gain-sqrt(2) initialisation (std sqrt(2 / fan_in): the maps keep their size
    through the stack), every bias non-zero.  Not orthogonal_: its QR is not reproducible across machines."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for name, (cin, cout, *_r) in zip(layer_names(kind), STACKS[kind][1]):
        P[name + ".weight"] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
        P[name + ".bias"] = 0.1 * torch.randn(cout, generator=g)
    return {k: v.numpy().astype(np.float32) for k, v in P.items()}


def convstack_data(kind, B, seed, u8=True):
    """Seeded inputs: 'image' (uint8, or those bytes / 255 as fp32; the occupancy map is 0 | 255 with a third of the cells set)
    and 'd_feat' (B, 1152 | 288) fp32."""
    r = np.random.default_rng(seed + 1_000_003)
    shape = (B,) + STACKS[kind][0]
    img = ((r.random(shape) < 0.3) * 255).astype(np.uint8) if kind == 2 else r.integers(0, 256, size=shape, dtype=np.uint8)
    d_feat = r.normal(size=(B, feat_width(kind))).astype(np.float32)
    return {"image": img if u8 else as_float_image(img), "d_feat": d_feat}


def as_float_image(img):
    """What the kernels read of a uint8 image: the byte divided by 255 in fp32."""
    img = np.asarray(img)
    return (img.astype(np.float32) / np.float32(255.0)) if img.dtype == np.uint8 else img.astype(np.float32)


def _windows(a):
    """(..., H, H) -> (..., H/2, H/2, 4): the cells of every 2 x 2 window in scan order."""
    return torch.stack([a[..., 0::2, 0::2], a[..., 0::2, 1::2], a[..., 1::2, 0::2], a[..., 1::2, 1::2]], -1)


def stack_forward(kind, P, x, gates=None, choices=None):
    """P: name -> tensor, x: (B, C, H, H) of the same dtype.  Returns (feat, acts, pre): acts / pre hold every convolution's
    un-pooled post-ReLU map / pre-activation by layer name.  gates: layer -> 0/1 tensor (z * gate replaces relu(z)); choices:
    pooled layer -> int64 tensor (B, C, H/2, H/2) of the chosen cell in scan order (replaces the maximum)."""
    acts, pre = {}, {}
    for name, (_cin, _cout, stride, pad, pooled) in zip(layer_names(kind), STACKS[kind][1]):
        z = F.conv2d(x, P[name + ".weight"], P[name + ".bias"], stride=stride, padding=pad)
        pre[name] = z
        a = torch.relu(z) if gates is None else z * gates[name]
        acts[name] = a
        if not pooled:
            x = a
        elif choices is None:
            x = F.max_pool2d(a, 2, 2)
        else:
            x = _windows(a).gather(-1, choices[name].unsqueeze(-1)).squeeze(-1)
    return x.flatten(1), acts, pre


def gates_of(arrays, kind):
    """layer -> bool array [activation > 0] from a dict holding 'act.<layer>'."""
    return {n: np.asarray(arrays["act." + n]) > 0 for n in layer_names(kind)}


def choices_of(arrays, kind):
    """pooled layer -> int64 array of each window's first maximum in scan order, from a dict holding 'act.<layer>'."""
    out = {}
    for n, (*_r, pooled) in zip(layer_names(kind), STACKS[kind][1]):
        if pooled:
            out[n] = _windows(torch.from_numpy(np.ascontiguousarray(arrays["act." + n]))).numpy().argmax(-1)
    return out


def evaluate(kind, P, d, dtype, gates=None, choices=None):
    """{'feat', 'act.<layer>', 'pre.<layer>', 'd.<parameter>'} on the CPU in `dtype`, as float64 numpy arrays: the forward over
    d['image'] (uint8 is divided by 255 in fp32 first, as the kernels do) and the gradients of sum(feat * d['d_feat'])."""
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dtype)   # noqa: E731
    Pt = {k: tt(P[k]).requires_grad_() for k in param_names(kind)}
    gt = None if gates is None else {k: tt(np.asarray(v, dtype=np.float64)) for k, v in gates.items()}
    ct = None if choices is None else {k: torch.from_numpy(np.ascontiguousarray(v)).long() for k, v in choices.items()}
    feat, acts, pre = stack_forward(kind, Pt, tt(as_float_image(d["image"])), gt, ct)
    grads = torch.autograd.grad((feat * tt(d["d_feat"])).sum(), list(Pt.values()))
    res = {"feat": feat}
    for n in layer_names(kind):
        res["act." + n], res["pre." + n] = acts[n], pre[n]
    res.update({"d." + k: g for k, g in zip(Pt, grads)})
    return {k: v.detach().double().numpy() for k, v in res.items()}


def same_units(a, b, kind):
    """Whether two results have identical gates and identical pool choices."""
    ga, gb, ca, cb = gates_of(a, kind), gates_of(b, kind), choices_of(a, kind), choices_of(b, kind)
    return all(np.array_equal(ga[k], gb[k]) for k in ga) and all(np.array_equal(ca[k], cb[k]) for k in ca)


_CASES = {}


def case(kind, B, seed):
    """(P, d, float64 evaluation, fp32 evaluation) of one seed, computed once per process (d holds the uint8 image)."""
    key = (kind, B, seed)
    if key not in _CASES:
        P, d = convstack_params(kind, seed), convstack_data(kind, B, seed)
        _CASES[key] = (P, d, evaluate(kind, P, d, torch.float64), evaluate(kind, P, d, torch.float32))
    return _CASES[key]


def forget(kind, B, keep_seed=None):
    """Drop the cached cases of a shape (their maps are large), all but `keep_seed`."""
    for key in [k for k in _CASES if k[:2] == (kind, B) and k[2] != keep_seed]:
        del _CASES[key]


def find_seed(kind, B, base_seed):
    """The first seed >= base_seed at which torch's fp32 CPU evaluation has the float64 evaluation's gates and pool choices."""
    for seed in range(base_seed, base_seed + 16):
        _P, _d, r64, r32 = case(kind, B, seed)
        if same_units(r64, r32, kind):
            return seed
        del _CASES[(kind, B, seed)]
    raise AssertionError("no seed with identical fp32 / float64 gates and pool choices in 16 tries")


COMPARED = ("feat", "act.", "d.")
CASE_SEED = 453


def draws_for(B):
    """20 draws up to B = 5; beyond, the float64 evaluations of the image stacks take seconds each: 3."""
    return 20 if B <= 5 else 3


def with_sums(r):
    """The compared arrays of a result, every weight gradient also as '<name>.rowsum' / '.colsum': its float64 sums over an output
    channel's (ci, ky, kx) and over the output channels -- the arrays a fixture keeps of it."""
    out = {}
    for k, a in r.items():
        if not k.startswith(COMPARED):
            continue
        a = np.asarray(a, dtype=np.float64)                       # (the sums below are float64 sums, whatever computed the array)
        out[k] = a
        if k.startswith("d.") and a.ndim == 4:
            m = a.reshape(a.shape[0], -1)
            out[k + ".rowsum"], out[k + ".colsum"] = m.sum(1), m.sum(0)
    return out


_DISTANCES = {}


def convstack_distance(kind, B, draws=None):
    """{array: distance}: per array, the largest over `draws` seeded draws (each the next seed without a flipped unit of the
    yardstick's own) of rel(torch fp32 CPU evaluation, float64 evaluation) at this shape.  Memoised per (kind, B); the first
    draw is the tests' own case (CASE_SEED's), which stays cached."""
    draws = draws_for(B) if draws is None else draws
    if (kind, B) in _DISTANCES and _DISTANCES[(kind, B)][0] >= draws:
        return _DISTANCES[(kind, B)][1]
    worst, seed, first = {}, CASE_SEED, None
    for _ in range(draws):
        seed = find_seed(kind, B, seed)
        first = seed if first is None else first
        _P, _d, r64, r32 = case(kind, B, seed)
        a64, a32 = with_sums(r64), with_sums(r32)
        for k in a64:
            worst[k] = max(worst.get(k, 0.0), rel(a32[k], a64[k]))
        forget(kind, B, keep_seed=first)
        seed += 1
    _DISTANCES[(kind, B)] = (draws, worst)
    return worst


def flipped_units(kind, got, ref, dist):
    """Units of `got` (a dict with 'act.<layer>') whose gate, or whose window's chosen cell, differs from the float64 forward
    `ref`'s: (count, the worst float64 margin / its allowance).  A flipped gate's margin is its |pre-activation|, a flipped
    choice's the difference of its two candidates' float64 values; the allowance is MARGIN * the layer's measured forward
    distance * the layer's largest magnitude."""
    count, worst = 0, 0.0
    gg, gr, cg, cr = gates_of(got, kind), gates_of(ref, kind), choices_of(got, kind), choices_of(ref, kind)
    for n in layer_names(kind):
        allow = MARGIN * dist["act." + n] * scale(ref["act." + n])
        flips = gg[n].reshape(gr[n].shape) != gr[n]
        if flips.any():
            count += int(flips.sum())
            worst = max(worst, float(np.abs(ref["pre." + n][flips]).max()) / allow)
        if n in cg:
            flips = cg[n] != cr[n]
            if flips.any():
                w = _windows(torch.from_numpy(np.ascontiguousarray(ref["act." + n]))).numpy()
                a = np.take_along_axis(w, cg[n][..., None], -1)[..., 0]
                b = np.take_along_axis(w, cr[n][..., None], -1)[..., 0]
                count += int(flips.sum())
                worst = max(worst, float(np.abs(a - b)[flips].max()) / allow)
    return count, worst


# ---- the fixtures made from the reference (tests/golden/make_golden_convstack.py) ------------------------------------------------
FIXTURE_B, FIXTURE_SEED, ROWS = 3, 453, 16
FIXTURES = {0: "convstack_kuka.npz", 1: "convstack_ithor.npz", 2: "convstack_occupancy.npz"}


@functools.lru_cache(maxsize=None)
def load_fixture(golden_dir, kind):
    return dict(np.load(os.path.join(golden_dir, FIXTURES[kind])))


def fixture_inputs(kind, g):
    """(P, d) of a fixture: the parameters are convstack_params at the fixture's seed (checked against the sums the file keeps of
    what the reference ran with), the data comes from the file."""
    P = convstack_params(kind, int(g["seed"].item()))
    for k in param_names(kind):
        assert np.array_equal(check_values(P[k]), g["check." + k]), k
    return P, {"image": g["image"], "d_feat": g["d_feat"].astype(np.float32)}


def fixture_distances(kind, got, g):
    """rel() of each array of `got` ('feat', 'd.<parameter>') from the fixture's.  A weight gradient gives three entries: every
    16th output-channel row under its own name, and '<name>.rowsum' / '.colsum', each relative to ITS largest magnitude."""
    res = {}
    for k, a in got.items():
        a = np.asarray(a, dtype=np.float64)
        if k == "feat":
            res[k] = rel(a, g["feat"])
        elif "g." + k in g:
            res[k] = rel(a, g["g." + k])
        elif "g." + k + ".rows16" in g:
            m = a.reshape(a.shape[0], -1)
            res[k] = rel(a[::ROWS], g["g." + k + ".rows16"])
            res[k + ".rowsum"] = rel(m.sum(1), g["g." + k + ".rowsum"])
            res[k + ".colsum"] = rel(m.sum(0), g["g." + k + ".colsum"])
    return res


# ---- a whole policy with the real stacks, for PPO.loss / PPO.update through bind_convs -----------------------------------------
# trunk_cpu's stand-in helpers with the stand-in stacks replaced by the real ones.  Q is the policy's named_parameters() as a dict
# of numpy arrays; gates / choices are keyed by parameter prefix ('base.imgCNN.0', 'base.occupancyCNNMLP.2', 'base.cnnMlp.0', ...).
from tests import trunk_cpu as tc  # noqa: E402

STACK_PREFIX = {0: ("base.imgCNN.",), 1: ("base.imgCNN.", "base.occupancyCNNMLP.")}


def policy_stacks(kind):
    """((prefix, stack kind, observation name), ...) of a base's convolution stacks."""
    return (("base.imgCNN.", kind, "image"),) + ((("base.occupancyCNNMLP.", 2, "occupancy"),) if kind else ())


def policy_params(kind, seed, n_act):
    """trunk_cpu.standin_params with the real stacks' convstack_params instead of the stand-in layers."""
    Q = {k: v for k, v in tc.standin_params(kind, seed, n_act).items()
         if not k.startswith(("base.imgCNN.", "base.occupancyCNNMLP.1."))}
    for prefix, sk, _obs in policy_stacks(kind):
        Q.update({prefix + k: v for k, v in convstack_params(sk, seed + 7 * sk).items()})
    return Q


def policy_forward(kind, Q, s, gates=None, choices=None):
    """Q, s: tensors of one dtype (images already divided by 255).  (value, actor_features, acts): the real stacks, then
    trunk_forward; acts / gates / choices by parameter prefix."""
    sub = lambda d, p, names: None if d is None else {n: d[p + n] for n in names if p + n in d}   # noqa: E731
    acts, outs = {}, {}
    for prefix, sk, obs in policy_stacks(kind):
        P = {k[len(prefix):]: v for k, v in Q.items() if k.startswith(prefix) and k[len(prefix):] in set(param_names(sk))}
        outs[obs], a, _pre = stack_forward(sk, P, s[obs], sub(gates, prefix, layer_names(sk)), sub(choices, prefix, layer_names(sk)))
        acts.update({prefix + n: v for n, v in a.items()})
    t = {"feat": outs["image"], "sound_in": s["goal_sound_feat"], "hxs": s["hxs"], "masks": s["masks"]}
    if kind:
        t["motor_in"], t["occ"] = s["image_feat"], outs["occupancy"]
    else:
        t["motor_in"] = torch.cat([s["image_feat"], s["robot_pose"]], 1)
    tg = None if gates is None else {n: gates["base." + n] for n, *_r, relu in tc.layers(kind) if relu}
    value, feats, _h, tacts, _pre = tc.trunk_forward(kind, {k[5:]: v for k, v in Q.items() if k.startswith("base.")}, t, tg)
    acts.update({"base." + n: tacts[n] for n, *_r in tc.layers(kind)})
    return value, feats, acts


def ppo_total(kind, Q, s, gates=None, choices=None):
    """The loss lines of models/ppo/algo/ppo.py:55-87 (clipped value loss) over the whole policy; returns (total, acts)."""
    values, feats, acts = policy_forward(kind, Q, s, gates, choices)
    dist = tc._dist(kind, Q, feats)
    logp = tc._logp(kind, dist, s["actions"])
    ratio = torch.exp(logp - s["old_logp"])
    action_loss = -torch.min(ratio * s["adv"], torch.clamp(ratio, 1.0 - tc.CLIP, 1.0 + tc.CLIP) * s["adv"]).mean()
    vpc = s["value_preds"] + (values - s["value_preds"]).clamp(-tc.CLIP, tc.CLIP)
    value_loss = 0.5 * torch.max((values - s["returns"]).pow(2), (vpc - s["returns"]).pow(2)).mean()
    return value_loss * tc.VCOEF + action_loss - dist.entropy().mean() * tc.ECOEF, acts


def ppo_sample(kind, Q, T, N, n_act, seed):
    """trunk_cpu.ppo_sample's minibatch with real observations: (3, 96, 96) uint8 images and the (1, 9, 9) occupancy map."""
    r = np.random.default_rng(seed)
    M, f = T * N, np.float32
    g = torch.Generator().manual_seed(seed)
    s = {"image": r.integers(0, 256, size=(M, 3, 96, 96), dtype=np.uint8), "image_feat": r.normal(size=(M, 3)).astype(f),
         "goal_sound_feat": r.normal(size=(M, 3)).astype(f), "hxs": (0.5 * r.normal(size=(N, tc.hidden(kind)))).astype(f),
         "masks": tc.trunk_masks(T, N, g).view(M, 1).numpy(), "adv": r.normal(size=(M, 1)).astype(f)}
    if kind:
        s["occupancy"] = ((r.random((M, 1, 9, 9)) < 0.3) * 255).astype(np.uint8)
    else:
        s["robot_pose"] = r.normal(size=(M, 2)).astype(f)
    with torch.no_grad():
        Q64, s64 = tc._tensors(Q, torch.float64), tc._tensors(s, torch.float64)
        values, feats, _ = policy_forward(kind, Q64, s64)
        dist = tc._dist(kind, Q64, feats)
        actions = dist.sample().unsqueeze(-1) if kind else dist.sample().float().double()
        logp = tc._logp(kind, dist, actions).numpy()
    values = values.numpy()
    sign = lambda: np.where(r.random((M, 1)) < 0.5, -1.0, 1.0)    # noqa: E731
    s["actions"] = actions.numpy() if kind else actions.numpy().astype(f)
    s["old_logp"] = (logp + sign() * r.uniform(0.01, 0.09, size=(M, 1))).astype(f)
    s["value_preds"] = (values + sign() * r.uniform(0.02, 0.15, size=(M, 1))).astype(f)
    s["returns"] = (values + sign() * r.uniform(0.5, 1.5, size=(M, 1))).astype(f)
    return s


def ppo_grads(kind, Q, s, dtype, gates=None, choices=None):
    """({parameter: gradient of the total, float64 numpy}, {prefix: activation}) on the CPU in `dtype`."""
    Qt = {k: v.requires_grad_() for k, v in tc._tensors(Q, dtype).items()}
    gt = None if gates is None else {k: torch.from_numpy(np.asarray(v, dtype=np.float64)).to(dtype) for k, v in gates.items()}
    ct = None if choices is None else {k: torch.from_numpy(np.ascontiguousarray(v)).long() for k, v in choices.items()}
    total, acts = ppo_total(kind, Qt, tc._tensors(s, dtype), gt, ct)
    grads = torch.autograd.grad(total, list(Qt.values()))
    return {k: g.double().numpy() for k, g in zip(Qt, grads)}, {k: v.detach().double().numpy() for k, v in acts.items()}


def policy_units(kind, acts):
    """(gates, choices) by parameter prefix from a dict of activations by prefix: every ReLU layer's gate, every pooled
    convolution's chosen cells."""
    gates, choices = {}, {}
    for prefix, sk, _obs in policy_stacks(kind):
        arrays = {"act." + n: acts[prefix + n] for n in layer_names(sk)}
        gates.update({prefix + n: v for n, v in gates_of(arrays, sk).items()})
        choices.update({prefix + n: v for n, v in choices_of(arrays, sk).items()})
    gates.update({"base." + n: np.asarray(acts["base." + n]) > 0 for n, *_r, relu in tc.layers(kind) if relu})
    return gates, choices


def count_unit_flips(a, b):
    """How many gates and pool choices differ between two policy_units results."""
    return sum(int((np.asarray(x[k]).reshape(np.asarray(y[k]).shape) != y[k]).sum()) for x, y in zip(a, b) for k in y)


_PPO = {}


def ppo_case(kind, T, N, n_act, seed):
    """(Q, s, float64 gradients, float64 activations, fp32 gradients, fp32 activations), once per process."""
    key = (kind, T, N, n_act, seed)
    if key not in _PPO:
        Q = policy_params(kind, seed, n_act)
        s = ppo_sample(kind, Q, T, N, n_act, seed + 500)
        _PPO[key] = (Q, s) + ppo_grads(kind, Q, s, torch.float64) + ppo_grads(kind, Q, s, torch.float32)
    return _PPO[key]


def find_ppo_seed(kind, T, N, n_act, base_seed):
    """The first seed at which the policy's fp32 CPU and float64 forwards have identical gates and pool choices."""
    for seed in range(base_seed, base_seed + 16):
        _Q, _s, _g64, a64, _g32, a32 = ppo_case(kind, T, N, n_act, seed)
        if count_unit_flips(policy_units(kind, a32), policy_units(kind, a64)) == 0:
            return seed
        del _PPO[(kind, T, N, n_act, seed)]
    raise AssertionError("no seed with identical fp32 / float64 gates and pool choices in 16 tries")


PPO_SEED = 60


@functools.lru_cache(maxsize=None)
def ppo_distance(kind, T, N, n_act, draws=None):
    """Per parameter of the policy, the largest over the draws (draws_for(T * N)) of rel(torch fp32 CPU gradient, float64
    gradient); the first draw is the tests' own case (PPO_SEED's), which stays cached."""
    draws = draws_for(T * N) if draws is None else draws
    worst, seed, first = {}, PPO_SEED, None
    for _ in range(draws):
        seed = find_ppo_seed(kind, T, N, n_act, seed)
        first = seed if first is None else first
        _Q, _s, g64, _a64, g32, _a32 = ppo_case(kind, T, N, n_act, seed)
        for k in g64:
            worst[k] = max(worst.get(k, 0.0), rel(g32[k], g64[k]))
        if seed != first:
            del _PPO[(kind, T, N, n_act, seed)]
        seed += 1
    return worst


def stack_module(kind, P):
    """An nn.Sequential with the reference's layers at the reference's indices (kind 2: occupancyCNNMLP whole, its Linear layers
    at 5 and 7) holding P: what conv_stack_eval takes as `module`.  No initialiser's values survive."""
    import torch.nn as nn
    mods = []
    for cin, cout, stride, pad, pooled in STACKS[kind][1]:
        mods += [nn.Conv2d(cin, cout, 3, stride=stride, padding=pad), nn.ReLU()] + ([nn.MaxPool2d(2, stride=2)] if pooled else [])
    mods.append(nn.Flatten())
    if kind == 2:
        mods += [nn.Linear(288, 128), nn.ReLU(), nn.Linear(128, 256), nn.ReLU()]
    seq = nn.Sequential(*mods)
    seq.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(P[k])) for k in param_names(kind)}, strict=kind != 2)
    return seq

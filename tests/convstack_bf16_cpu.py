"""CPU restatement of the convolution stacks' bf16 mode (include/var_hip.h, "flags bit 0"), LAYER BY LAYER: every convolution
product, in all three directions, multiplies operands rounded to bf16 (round to nearest even) and accumulates exactly (float64
here); everything stored is fp32; the bias is added unrounded; pools, ReLU gates and the pool backward are exact selections.

A product on rounded operands differs from the fp32 one by far more than any summation error, and a ReLU gate that falls the other
way would carry that difference through every layer above it.  So nothing here is compared end to end: each layer's forward map,
weight gradient, bias gradient and gated data gradient is recomputed in float64 FROM THE BUFFERS THE GPU RETURNED BELOW (or above)
IT -- `saved`, `grad_maps`, the parameters, the image -- and only that one product's rounding is left in the comparison.

Bounds (the rule of convstack_cpu.convstack_distance, per product): per compared array, four times the distance of torch's own
fp32 CPU evaluation of the SAME ROUNDED-OPERAND PRODUCT from its float64 evaluation, the largest over the draws (20 up to B = 5, 3
beyond), relative to the array's largest magnitude.  The operands of a draw come from this file's own fp32 chain at the draw's
seed.  The yardstick is torch against float64, never the kernel."""
import numpy as np
import torch
import torch.nn.functional as F

from tests import convstack_cpu as cc
from tests.gru_seq_cpu import rel, scale  # noqa: F401

MARGIN = 4.0


def bf16_round(t):
    """A tensor of fp32-representable values rounded to bf16 (nearest, ties to even), in its own dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def _r(t, rounding):
    return bf16_round(t) if rounding else t


def geometry(kind):
    """((name, cin, cout, stride, padding, pooled), ...) of a stack's convolutions."""
    return tuple((n,) + tuple(c) for n, c in zip(cc.layer_names(kind), cc.STACKS[kind][1]))


def tt(a, dtype=None):
    t = a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t if dtype is None else t.to(dtype)


# ---- one layer's products -------------------------------------------------------------------------------------------------------
def conv_forward(x, w, b, stride, pad, dtype, rounding=True):
    """relu(conv(bf16(x), bf16(w)) + b) in `dtype`."""
    return torch.relu(F.conv2d(_r(x, rounding).to(dtype), _r(w, rounding).to(dtype), b.to(dtype), stride=stride, padding=pad))


def weight_grad(x, g, wshape, stride, pad, dtype, rounding=True):
    """The sum over pixels of bf16(g) * bf16(x), (cout, cin, 3, 3)."""
    return torch.nn.grad.conv2d_weight(_r(x, rounding).to(dtype), tuple(wshape), _r(g, rounding).to(dtype), stride=stride, padding=pad)


def data_grad(g, w, xshape, stride, pad, dtype, rounding=True):
    """conv_transpose(bf16(g), bf16(w)), ungated, of the layer input's shape."""
    return torch.nn.grad.conv2d_input(tuple(xshape), _r(w, rounding).to(dtype), _r(g, rounding).to(dtype), stride=stride, padding=pad)


def bias_grad(g, dtype):
    return g.to(dtype).sum((0, 2, 3))


def pool(a):
    return F.max_pool2d(a, 2, 2)


def gate_below(dx, act_below, pooled):
    """The gradient with respect to the pre-activation of the layer below, from dx (the gradient with respect to this layer's
    input) and the layer below's un-pooled post-ReLU map: exact selections.  Unpooled: dx where the map is positive.  Pooled: a
    window's dx goes to its first maximum in scan order and is dropped where that maximum is not positive."""
    if not pooled:
        return dx * (act_below > 0).to(dx.dtype)
    w = cc._windows(act_below)
    best = w.argmax(-1)                                               # (the first of equal maxima)
    top = w.gather(-1, best.unsqueeze(-1)).squeeze(-1)
    gsel = torch.where(top > 0, dx, torch.zeros_like(dx))
    out = torch.zeros(act_below.shape, dtype=dx.dtype)
    for cell, (i, j) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[..., i::2, j::2] = gsel * (best == cell).to(dx.dtype)
    return out


# ---- the whole stack on its own buffers (rounding off: convstack_cpu.evaluate) ----------------------------------------------------
def chain(kind, P, d, dtype, rounding=True):
    """{'feat', 'act.<l>', 'g.<l>', 'd.<l>.weight', 'd.<l>.bias'} as tensors of `dtype`: every layer from the chain's own maps
    below it and gradients above it."""
    geo = geometry(kind)
    x = tt(cc.as_float_image(d["image"]), dtype)
    res, xs = {}, []
    for name, _cin, _cout, stride, pad, pooled in geo:
        xs.append(x)
        a = conv_forward(x, tt(P[name + ".weight"]), tt(P[name + ".bias"]), stride, pad, dtype, rounding)
        res["act." + name] = a
        x = pool(a) if pooled else a
    res["feat"] = x.flatten(1)
    last = geo[-1][0]
    g = tt(d["d_feat"], dtype).reshape(res["act." + last].shape) * (res["act." + last] > 0).to(dtype)
    for l in range(len(geo) - 1, -1, -1):
        name, _cin, _cout, stride, pad, _pooled = geo[l]
        res["g." + name] = g
        w = tt(P[name + ".weight"])
        res["d." + name + ".weight"] = weight_grad(xs[l], g, w.shape, stride, pad, dtype, rounding)
        res["d." + name + ".bias"] = bias_grad(g, dtype)
        if l:
            dx = data_grad(g, w, xs[l].shape, stride, pad, dtype, rounding)
            g = gate_below(dx, res["act." + geo[l - 1][0]], geo[l - 1][5])
    return res


# ---- per-layer float64 references from the GPU's own buffers ----------------------------------------------------------------------
def layer_inputs(kind, image, acts, images=None):
    """x_l per layer as fp32 tensors: the float image, or the (pooled) fp32 map below.  images: a list of image indices to keep."""
    geo = geometry(kind)
    pick = (lambda a: a) if images is None else (lambda a: a[images])
    xs = [pick(tt(cc.as_float_image(image)))]
    for name, *_r3, pooled in geo[:-1]:
        a = pick(tt(acts["act." + name], torch.float32))
        xs.append(pool(a) if pooled else a)
    return xs


def layer_refs(kind, P, d, got, images=None, what=("act", "g", "w", "b"), layers=None, rounding=True):
    """Float64 references of the arrays in `got` ('act.<l>', 'g.<l>' as fp32 numpy arrays from the GPU): 'act.<l>' from the GPU's
    map below, 'g.<l>' (l below the last) from the GPU's g of the layer above and the GPU's map of layer l, 'g.<last>' from d_feat,
    'd.<l>.weight' / '.bias' from the GPU's g_l and x_l.  images: restrict the per-image arrays ('act', 'g') to these images.
    rounding=False: the same products on unrounded operands (the fp32 mode's references)."""
    geo = geometry(kind)
    names = [n for n, *_ in geo]
    layers = names if layers is None else layers
    f64 = torch.float64
    pick = (lambda a: a) if images is None else (lambda a: a[images])
    ref = {}
    xs = layer_inputs(kind, d["image"], got, images)
    xs_all = xs if images is None else None
    for l, (name, _cin, _cout, stride, pad, _pooled) in enumerate(geo):
        if name not in layers:
            continue
        w, b = tt(P[name + ".weight"]), tt(P[name + ".bias"])
        if "act" in what:
            ref["act." + name] = conv_forward(xs[l], w, b, stride, pad, f64, rounding)
        if "g" in what:
            if l == len(geo) - 1:
                a = pick(tt(got["act." + name], torch.float32))
                ref["g." + name] = pick(tt(d["d_feat"], f64)).reshape(a.shape) * (a > 0).to(f64)
            else:
                up, _ci, _co, s2, p2, _pl = geo[l + 1]
                dx = data_grad(pick(tt(got["g." + up], torch.float32)), tt(P[up + ".weight"]), xs[l + 1].shape, s2, p2, f64,
                               rounding)
                ref["g." + name] = gate_below(dx, pick(tt(got["act." + name], torch.float32)), geo[l][5])
        if "w" in what or "b" in what:
            if xs_all is None:
                xs_all = layer_inputs(kind, d["image"], got)
            g = tt(got["g." + name], torch.float32)
            if "w" in what:
                ref["d." + name + ".weight"] = weight_grad(xs_all[l], g, w.shape, stride, pad, f64, rounding)
            if "b" in what:
                ref["d." + name + ".bias"] = bias_grad(g, f64)
    return {k: v.numpy() for k, v in ref.items()}


def nontrivial(kind, res):
    """The condition the GPU tests assert of a case: every post-ReLU map has positive units and zero units, every compared
    gradient array a non-zero largest magnitude.  res: 'act.<l>', 'g.<l>', 'd.<l>.*' (tensors or arrays)."""
    for name, *_ in geometry(kind):
        a = np.asarray(res["act." + name])
        if not ((a > 0).any() and (a == 0).any()):
            return False
        for k in ("g." + name, "d." + name + ".weight", "d." + name + ".bias"):
            if not np.abs(np.asarray(res[k])).max() > 0:
                return False
    return True


# ---- the bounds ---------------------------------------------------------------------------------------------------------------------
CASE_SEED = 611
_BOUNDS = {}


def draws_for(B):
    return 20 if B <= 5 else 3


def product_distances(kind, ops, rounding=True):
    """{array: rel(torch fp32 CPU evaluation, float64 evaluation)} of every layer's rounded-operand products (rounding=False: the
    same products on unrounded operands) over the operands `ops` (a chain() result: x_l from its maps, g_l its gradients)."""
    geo = geometry(kind)
    f32, f64 = torch.float32, torch.float64
    image = ops["image"]
    xs = layer_inputs(kind, image, {k: v for k, v in ops.items() if k.startswith("act.")})
    out = {}
    for l, (name, _cin, _cout, stride, pad, _pooled) in enumerate(geo):
        w, b, g = ops["P"][name + ".weight"], ops["P"][name + ".bias"], ops["g." + name].float()
        out["act." + name] = rel(conv_forward(xs[l], w, b, stride, pad, f32, rounding).numpy(),
                                  conv_forward(xs[l], w, b, stride, pad, f64, rounding).numpy())
        out["d." + name + ".weight"] = rel(weight_grad(xs[l], g, w.shape, stride, pad, f32, rounding).numpy(),
                                           weight_grad(xs[l], g, w.shape, stride, pad, f64, rounding).numpy())
        out["d." + name + ".bias"] = rel(bias_grad(g, f32).numpy(), bias_grad(g, f64).numpy())
        if l:
            below = ops["act." + geo[l - 1][0]].float()
            a32 = gate_below(data_grad(g, w, xs[l].shape, stride, pad, f32, rounding), below, geo[l - 1][5])
            a64 = gate_below(data_grad(g, w, xs[l].shape, stride, pad, f64, rounding), below, geo[l - 1][5])
            out["g." + geo[l - 1][0]] = rel(a32.numpy(), a64.numpy())
    out["g." + geo[-1][0]] = 0.0                                      # the last layer's gate is a selection of d_feat: exact
    return out


def draw_operands(kind, B, seed, rounding=True):
    P, d = cc.convstack_params(kind, seed), cc.convstack_data(kind, B, seed)
    ops = chain(kind, P, d, torch.float32, rounding)
    ops["P"] = {k: tt(v) for k, v in P.items()}
    ops["image"] = d["image"]
    return ops


def bounds(kind, B, draws=None, rounding=True):
    """{array: MARGIN * the largest product_distances over the draws at this shape}; memoised per (kind, B, rounding)."""
    draws = draws_for(B) if draws is None else draws
    key = (kind, B, rounding)
    if key not in _BOUNDS or _BOUNDS[key][0] < draws:
        worst = {}
        for i in range(draws):
            for k, v in product_distances(kind, draw_operands(kind, B, CASE_SEED + i, rounding), rounding).items():
                worst[k] = max(worst.get(k, 0.0), v)
        _BOUNDS[key] = (draws, {k: MARGIN * v for k, v in worst.items()})
    return _BOUNDS[key][1]


def weight_grad_bound(kind, B, name, draws=3, rounding=True):
    """MARGIN * the largest distance of one layer's weight gradient over `draws` draws at batch B (the grid-wrap sizes: the whole
    chain in float64 would take minutes there).  A draw's x_l is the fp32 chain's forward up to that layer; its g_l is a seeded
    Gaussian map gated by the layer's own ReLU pattern: the fp32-against-float64 distance of a sum depends on the number and spread
    of its terms, not on which loss produced g."""
    geo = geometry(kind)
    l = [n for n, *_ in geo].index(name)
    _n, _cin, _cout, stride, pad, _pooled = geo[l]
    worst = 0.0
    for i in range(draws):
        P, d = cc.convstack_params(kind, CASE_SEED + i), cc.convstack_data(kind, B, CASE_SEED + i)
        x = tt(cc.as_float_image(d["image"]))
        for nm, _ci, _co, s2, p2, pooled in geo[:l]:
            a = conv_forward(x, tt(P[nm + ".weight"]), tt(P[nm + ".bias"]), s2, p2, torch.float32, rounding)
            x = pool(a) if pooled else a
        w = tt(P[name + ".weight"])
        a = conv_forward(x, w, tt(P[name + ".bias"]), stride, pad, torch.float32, rounding)
        g = torch.randn(a.shape, generator=torch.Generator().manual_seed(CASE_SEED + i)) * (a > 0).float()
        worst = max(worst, rel(weight_grad(x, g, w.shape, stride, pad, torch.float32, rounding).numpy(),
                               weight_grad(x, g, w.shape, stride, pad, torch.float64, rounding).numpy()))
    return MARGIN * worst


# ---- the cases of tests/test_gpu_convstack_bf16.py (the host file checks each of them for non-triviality) ---------------------------
PARITY_CASES = [(k, B, True) for k in (0, 1) for B in (1, 2, 3, 5)] + [(k, 2, False) for k in (0, 1)]
PARITY_SEED = 77


def all_bytes_case(kind, seed=PARITY_SEED):
    """(P, d) at B = 1 whose image holds all 256 byte values (a seeded permutation of i mod 256 over the pixels)."""
    P, d = cc.convstack_params(kind, seed), cc.convstack_data(kind, 1, seed)
    n = d["image"].size
    d["image"] = (np.random.default_rng(seed).permutation(n) % 256).astype(np.uint8).reshape(d["image"].shape)
    assert len(np.unique(d["image"])) == 256
    return P, d

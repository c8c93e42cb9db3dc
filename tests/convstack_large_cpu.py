"""Support of the convolution stacks' checks at the batch sizes the PPO update runs (tests/test_convstack_large_host.py,
tests/test_gpu_convstack_large.py).  CPU only.

1.  A restatement of csrc/convstack.hip's wgrad_split and layout_of (fp32 mode) in Python.  The GPU file's case table is built
    from it: both sides of the first batch size at which a layer's split cap holds, the update's shapes, the documented limit.
2.  Repeated-image cases.  Image b of a batch is distinct[b % R]; d_feat is drawn fresh for every b.  A layer's input x_l is then
    the same for all copies of an image, and its weight gradient is linear in the copies' g_l:
        dW_l = sum_b x_b (*) g_b = sum_{i < R} x_i (*) (sum_{b = i mod R} g_b),
    so the float64 reference of a B-image weight gradient costs an R-image one.  The kernel cannot tell that images repeat: every
    product g * x still differs between copies, because g does.
3.  The yardstick at these shapes (the rule of convstack_bf16_cpu): per array four times the distance of torch's fp32 CPU
    evaluation of the same full-shape product from float64, the largest over the draws, relative to the array's largest magnitude.
    Operands as convstack_bf16_cpu.weight_grad_bound builds them (fp32 chain forward, seeded Gaussian g gated by the layer's own
    ReLU pattern), with repeated images.  The yardstick is torch against float64, never the kernel.
4.  A stand-in of the kernels' split structure in torch fp32 that takes injected faults, and emulations of the bias sum's and the
    fold's own order of additions in fp32.
5.  The gather-GEMM's one-accumulator K chain of the forward and the data gradient emulated in fp32, and the bound of the three
    rows that are held to it."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
import torch.nn.functional as F

from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc

# ---- 1: csrc/convstack.hip's split and workspace arithmetic ------------------------------------------------------------------------
GG_MT = 128             # gg.h: rows of a tile
WGRAD_KC = 32           # kWgradKC: pixels per K chunk of a weight gradient
CHAN_CHUNKS = 32        # kChanChunks: partial sums per channel of a bias gradient
WIDE_FOLD = 4096        # kWideFold
WIDE_SLABS = 128        # kWideSlabs
SMALL_IMAGES = 8        # kSmallImages
MAX_BATCH = 1024        # kMaxBatch
TESTED_BEFORE = 25      # the largest batch of tests/test_gpu_convstack.py's float64 pins before this file
UPDATE_SHAPES = {0: (200, 400), 1: (200,), 2: (200,)}    # DESIGN.md, "The PPO update's convolution stacks"


def is_small(kind):
    return kind == 2


def shapes_of(kind):
    """[(hin, hout)] per convolution: shapes_of() of convstack.hip."""
    (_c, h, _w), convs = cc.STACKS[kind]
    out = []
    for _cin, _cout, stride, pad, pooled in convs:
        ho = (h + 2 * pad - 3) // stride + 1
        out.append((h, ho))
        h = ho // 2 if pooled else ho
    return out


def act_floats(kind, l):
    return cc.STACKS[kind][1][l][1] * shapes_of(kind)[l][1] ** 2


def wgrad_plan(kind, l, B):
    """wgrad_split() of convstack.hip with what it passes through: {'tiles', 'kchunks', 'cap', 'splits', 'per', 'last'} -- the
    layer's split cap (1024 / tiles, at most kWideSlabs for a gradient of kWideFold floats or more), the split count at batch B,
    the 32-pixel chunks per split and those of the last split.  Kind 2: slabs of kSmallImages images ('per' and 'last' in images)."""
    cin, cout = cc.STACKS[kind][1][l][:2]
    if is_small(kind):
        ns = (B + SMALL_IMAGES - 1) // SMALL_IMAGES
        return {"tiles": 0, "kchunks": B, "cap": MAX_BATCH // SMALL_IMAGES, "splits": ns, "per": SMALL_IMAGES,
                "last": B - (ns - 1) * SMALL_IMAGES}
    M, N = cin * 9, cout
    K = B * shapes_of(kind)[l][1] ** 2
    tiles = ((M + GG_MT - 1) // GG_MT) * ((N + 63) // 64)
    kchunks = (K + WGRAD_KC - 1) // WGRAD_KC
    cap = (1024 + tiles - 1) // tiles
    if M * N >= WIDE_FOLD and cap > WIDE_SLABS:
        cap = WIDE_SLABS
    ns = max(1, min(cap, kchunks // 4))
    per = (kchunks + ns - 1) // ns
    splits = (kchunks + per - 1) // per
    return {"tiles": tiles, "kchunks": kchunks, "cap": cap, "splits": splits, "per": per, "last": kchunks - (splits - 1) * per}


def wgrad_split(kind, l, B):
    return wgrad_plan(kind, l, B)["splits"]


def cap_holds(kind, l, B):
    """Whether the layer's cap, not the quarter of its K chunks, limits the split count at batch B (kind 2: the slab count has
    reached its cap)."""
    p = wgrad_plan(kind, l, B)
    return p["splits"] >= p["cap"] if is_small(kind) else p["kchunks"] // 4 >= p["cap"]


def first_cap_batch(kind, l):
    """The first B at which the layer's cap holds (it holds from there on: kchunks grows with B); None where that is above
    kMaxBatch."""
    for B in range(1, MAX_BATCH + 1):
        if cap_holds(kind, l, B):
            return B
    return None


def layout_total_floats(kind, B):
    """layout_of(st, B).total of convstack.hip, fp32 mode, in floats."""
    up4 = lambda n: (n + 3) & ~3                                      # noqa: E731
    convs = cc.STACKS[kind][1]
    max_act = max_pool = max_slab = saved = 0
    for l, (cin, cout, _s, _p, pooled) in enumerate(convs):
        a = B * act_floats(kind, l)
        saved += a
        max_act = max(max_act, a)
        if pooled:
            max_pool = max(max_pool, a // 4)
        max_slab = max(max_slab, wgrad_split(kind, l, B) * cin * 9 * cout)
    o = up4(max_pool)
    fwd_base = o
    o += 2 * up4(max_act) + up4(max_pool) + up4(max_slab) + CHAN_CHUNKS * 256
    return max(o, fwd_base + up4(saved))


def chan_sum_chain(kind, l, B):
    """Elements a thread of cs_chan_sum_kernel adds in index order at batch B (the longest thread of a chunk)."""
    tot = B * shapes_of(kind)[l][1] ** 2
    per = (tot + CHAN_CHUNKS - 1) // CHAN_CHUNKS
    return (per + 255) // 256


# bf16 mode: which layers img_bf16.hip's kernels divert from the gather-GEMM (t2_candidate() of convstack.hip and the shapes
# c3_by_shape / img_bf16_wgrad_slab_floats cover: (cin, cout, side of the map))
T2_CONV_SHAPES = {(32, 32, 96), (32, 64, 48), (64, 64, 24), (64, 128, 12), (64, 64, 48), (64, 128, 24), (128, 128, 24)}
T2_WGRAD_SHAPES = {(32, 32, 96), (32, 64, 48), (64, 64, 48)}


def _t2(kind, l, shapes):
    cin, cout, stride, pad, _pooled = cc.STACKS[kind][1][l]
    return not is_small(kind) and l > 0 and stride == 1 and pad == 1 and (cin, cout, shapes_of(kind)[l][0]) in shapes


def gemm_layers(kind, precision, what):
    """Names of the layers whose forward and data gradient (what = 'conv') or weight gradient ('wgrad') the gather-GEMM (kind 2:
    the small kernels) serves in a precision: all of them in fp32, those img_bf16.hip does not divert in bf16."""
    names = cc.layer_names(kind)
    if precision == "fp32":
        return tuple(names)
    shapes = T2_CONV_SHAPES if what == "conv" else T2_WGRAD_SHAPES
    return tuple(n for l, n in enumerate(names) if not _t2(kind, l, shapes))


def cases():
    """[(kind, B, layers)] of tests/test_gpu_convstack_large.py: both sides of every first-cap size above the sizes tested before
    (that layer's gradients), the update's shapes and the limit (all layers); kind 2 at its update shape, the limit and one below
    it (a ragged last slab)."""
    out = []
    for kind in (0, 1):
        names = cc.layer_names(kind)
        for l, n in enumerate(names):
            first = first_cap_batch(kind, l)
            if first is not None and first > TESTED_BEFORE:
                out += [(kind, first - 1, (n,)), (kind, first, (n,))]
        out += [(kind, B, tuple(names)) for B in UPDATE_SHAPES[kind] + (MAX_BATCH,)]
    out += [(2, B, tuple(cc.layer_names(2))) for B in UPDATE_SHAPES[2] + (MAX_BATCH - 1, MAX_BATCH)]
    return out


def describe(kind, B, layers):
    """One line per layer of a case: split count and chunks per split."""
    names = cc.layer_names(kind)
    rows = []
    for n in layers:
        p = wgrad_plan(kind, names.index(n), B)
        rows.append(f"kind {kind} B {B} layer {n}: cap {p['cap']}, {p['splits']} splits of {p['per']} "
                    f"{'images' if is_small(kind) else 'chunks'} (the last {p['last']}), bias threads add "
                    f"{chan_sum_chain(kind, names.index(n), B)} elements")
    return rows


# ---- 2: repeated-image cases ---------------------------------------------------------------------------------------------------------
R_DEFAULT = 8
LARGE_SEED = 1300


def repeated_data(kind, B, seed, R=R_DEFAULT):
    """{'image' (B, ...) uint8 with image b = distinct[b % R], 'd_feat' (B, width) fp32 drawn fresh for every b, 'distinct'}."""
    distinct = cc.convstack_data(kind, R, seed)["image"]
    d_feat = np.random.default_rng(seed + 2_000_003).normal(size=(B, cc.feat_width(kind))).astype(np.float32)
    return {"image": distinct[np.arange(B) % R], "d_feat": d_feat, "distinct": distinct}


def copy_sums(g, R, rounding=False, chunk=64):
    """(R, ...) float64: sum over the copies b = i mod R of g_b (rounded to bf16 first where the product rounds it), accumulated in
    float64."""
    g = cb.tt(g)
    out = torch.zeros((R,) + tuple(g.shape[1:]), dtype=torch.float64)
    for b0 in range(0, g.shape[0], chunk):
        part = g[b0:b0 + chunk]
        out.index_add_(0, torch.arange(b0, b0 + part.shape[0]) % R, cb._r(part.float(), rounding).double())
    return out


def reduced_weight_grad(x_R, gsum, wshape, stride, pad, rounding=False):
    """The float64 weight gradient of a repeated-image batch from its R distinct inputs and the copies' summed gradients."""
    return cb.weight_grad(cb._r(cb.tt(x_R).float(), rounding).double(), gsum, wshape, stride, pad, torch.float64, rounding=False)


def sums_of(name, w):
    """{name, name.rowsum, name.colsum}: convstack_cpu.with_sums for one weight gradient."""
    return cc.with_sums({name: np.asarray(w)})


# ---- 3: the yardstick ------------------------------------------------------------------------------------------------------------------
_DIST = {}


def draws_for(B):
    """3 up to B = 409; above (807 and more) one: a draw's full-shape fp32 products of a whole stack take seconds there."""
    return 3 if B <= 409 else 1


def gaussian(shape, seed, block=16):
    """(B, ...) fp32 standard normal, a function of (shape, seed) alone: blocks of `block` images, each from its own generator, filled
    by a thread pool."""
    out = np.empty(shape, dtype=np.float32)

    def fill(b0):
        np.random.default_rng([seed, b0]).standard_normal(out=out[b0:b0 + block], dtype=np.float32)

    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as ex:
        list(ex.map(fill, range(0, shape[0], block)))
    return torch.from_numpy(out)


def draw_layer_operands(kind, B, seed, layers, rounding, R=R_DEFAULT):
    """Per layer of `layers`: (x_R, g) -- the fp32 chain's input of the layer over the R distinct images and a seeded Gaussian
    (B, ...) map gated by the ReLU pattern of the layer's own map at image b % R.  A generator: one layer's arrays at a time."""
    geo = cb.geometry(kind)
    P = cc.convstack_params(kind, seed)
    x = cb.tt(cc.as_float_image(cc.convstack_data(kind, R, seed)["image"]))
    idx = torch.arange(B) % R
    for l, (name, _ci, _co, stride, pad, pooled) in enumerate(geo):
        a = cb.conv_forward(x, cb.tt(P[name + ".weight"]), cb.tt(P[name + ".bias"]), stride, pad, torch.float32, rounding)
        if name in layers:
            g = gaussian((B,) + tuple(a.shape[1:]), seed * 100 + l)
            g *= (a > 0).float()[idx]
            yield name, l, x, g
        x = cb.pool(a) if pooled else a


def layer_distances(kind, l, x_R, g, rounding, R=R_DEFAULT):
    """{array: rel(torch fp32 CPU evaluation at the full shape, float64)} of one layer's weight gradient (with its float64 row and
    column sums) and bias gradient over the operands (x_R, g)."""
    name, _ci, cout, stride, pad, _pl = cb.geometry(kind)[l]
    wshape = (cout, x_R.shape[1], 3, 3)
    B = g.shape[0]
    w32 = cb.weight_grad(x_R[torch.arange(B) % R], g, wshape, stride, pad, torch.float32, rounding).numpy()
    gs = copy_sums(g, R, rounding)
    w64 = reduced_weight_grad(x_R, gs, wshape, stride, pad, rounding).numpy()
    key = "d." + name + ".weight"
    a32, a64 = sums_of(key, w32), sums_of(key, w64)
    out = {k: cb.rel(a32[k], a64[k]) for k in a64}
    b64 = (gs if not rounding else copy_sums(g, R, False)).sum((0, 2, 3)).numpy()
    out["d." + name + ".bias"] = cb.rel(cb.bias_grad(g, torch.float32).numpy(), b64)
    return out


def large_distances(kind, B, layers, rounding=False, draws=None, R=R_DEFAULT):
    """{array: the largest layer_distances over the draws} for the layers named; memoised per (kind, B, layer, rounding)."""
    draws = draws_for(B) if draws is None else draws
    todo = [n for n in layers if _DIST.get((kind, B, n, rounding, R), (0,))[0] < draws]
    if todo:
        worst = {n: {} for n in todo}
        for i in range(draws):
            for name, l, x_R, g in draw_layer_operands(kind, B, cb.CASE_SEED + i, todo, rounding, R):
                for k, v in layer_distances(kind, l, x_R, g, rounding, R).items():
                    worst[name][k] = max(worst[name].get(k, 0.0), v)
        for n in todo:
            _DIST[(kind, B, n, rounding, R)] = (draws, worst[n])
    out = {}
    for n in layers:
        out.update(_DIST[(kind, B, n, rounding, R)][1])
    return out


def large_bounds(kind, B, layers, rounding=False, draws=None, R=R_DEFAULT):
    return {k: cb.MARGIN * v for k, v in large_distances(kind, B, layers, rounding, draws, R).items()}


# ---- 4: a stand-in of the split structure, with faults; the kernels' own order of additions ---------------------------------------------
FAULTS = ("drop_chunk", "double_chunk", "drop_ragged_split", "skip_last_slab", "drop_bias_chunk", "shifted_copy")


def standin(kind, l, x_R, g, fault=None, R=R_DEFAULT, at=None):
    """torch's fp32 evaluation of layer l's weight and bias gradient in the kernels' STRUCTURE -- K = (b, oy, ox) cut into 32-pixel
    chunks, the chunks into wgrad_plan's splits, one slab per split, the slabs added in slab order; the bias as kChanChunks partial
    sums per channel added in chunk order -- with one fault injected:
      drop_chunk / double_chunk   chunk `at` (default: the middle chunk of the last but one split) left out / counted twice
      drop_ragged_split           the last split computes nothing (its slab is zero)
      skip_last_slab              the fold stops one slab early
      drop_bias_chunk             chunk `at` (default 17) of every channel's bias sum left out
      shifted_copy                image `at` (default R + 1) takes its g from the copy R places further on
    Returns {'d.<l>.weight', its row and column sums, 'd.<l>.bias'} as numpy arrays."""
    name, _ci, cout, stride, pad, _pl = cb.geometry(kind)[l]
    B = g.shape[0]
    plan = wgrad_plan(kind, l, B)
    if fault == "shifted_copy":
        at = R + 1 if at is None else at
        g = g.clone()
        g[at] = g[at + R]
    cols = F.unfold(x_R, 3, padding=pad, stride=stride)                                  # (R, cin * 9, pixels)
    A = cols[torch.arange(B) % R].permute(1, 0, 2).reshape(cols.shape[1], -1)             # (M, K), k = (b, oy, ox)
    G = g.reshape(B, cout, -1).permute(1, 0, 2).reshape(cout, -1)                          # (N, K)
    K = A.shape[1]
    assert plan["kchunks"] == (K + WGRAD_KC - 1) // WGRAD_KC
    if at is None or fault not in ("drop_chunk", "double_chunk"):
        chunk_at = (plan["splits"] - 2) * plan["per"] + plan["per"] // 2
    else:
        chunk_at = at
    slabs = []
    for s in range(plan["splits"]):
        c_lo, c_hi = s * plan["per"], min(plan["kchunks"], (s + 1) * plan["per"])
        k_lo, k_hi = c_lo * WGRAD_KC, min(K, c_hi * WGRAD_KC)
        slab = G[:, k_lo:k_hi] @ A[:, k_lo:k_hi].T
        if fault in ("drop_chunk", "double_chunk") and c_lo <= chunk_at < c_hi:
            ks = slice(chunk_at * WGRAD_KC, min(K, (chunk_at + 1) * WGRAD_KC))
            extra = G[:, ks] @ A[:, ks].T
            slab = slab - extra if fault == "drop_chunk" else slab + extra
        if fault == "drop_ragged_split" and s == plan["splits"] - 1:
            slab = torch.zeros_like(slab)
        slabs.append(slab)
    if fault == "skip_last_slab":
        slabs = slabs[:-1]
    w = torch.zeros_like(slabs[0])
    for slab in slabs:
        w = w + slab
    out = sums_of("d." + name + ".weight", w.reshape(cout, -1, 3, 3).numpy())
    flat = G                                                                             # per channel, e = b * inner + i
    per = (K + CHAN_CHUNKS - 1) // CHAN_CHUNKS
    bias = torch.zeros(cout)
    for j in range(CHAN_CHUNKS):
        if fault == "drop_bias_chunk" and j == (17 if at is None else at):
            continue
        bias = bias + flat[:, j * per:min(K, (j + 1) * per)].sum(1)
    out["d." + name + ".bias"] = bias.numpy()
    return out


def reference(kind, l, x_R, g, R=R_DEFAULT, rounding=False):
    """The reduced float64 reference of the same arrays."""
    name, _ci, cout, stride, pad, _pl = cb.geometry(kind)[l]
    gs = copy_sums(g, R, rounding)
    out = sums_of("d." + name + ".weight", reduced_weight_grad(x_R, gs, (cout, x_R.shape[1], 3, 3), stride, pad, rounding).numpy())
    out["d." + name + ".bias"] = (gs if not rounding else copy_sums(g, R, False)).sum((0, 2, 3)).numpy()
    return out


def emulate_chan_sum(g, chunks=CHAN_CHUNKS):
    """cs_chan_sum_kernel's own order in fp32 over g (C, tot), the channels' elements in e = b * inner + i order: per chunk a
    thread adds its elements e = lo + t, lo + t + 256, ... in order, then the 256 sums as the kernel's tree.  (chunks, C) fp32."""
    g = np.ascontiguousarray(g, dtype=np.float32)
    C, tot = g.shape
    per = (tot + chunks - 1) // chunks
    iters = (per + 255) // 256
    part = np.zeros((chunks, C), dtype=np.float32)
    for j in range(chunks):
        lo, hi = j * per, min(tot, (j + 1) * per)
        if lo >= hi:
            continue
        pad = np.zeros((C, iters * 256), dtype=np.float32)
        pad[:, :hi - lo] = g[:, lo:hi]                                # (adding the zeros behind a thread's last element is exact)
        pad = pad.reshape(C, iters, 256)
        acc = np.zeros((C, 256), dtype=np.float32)
        for it in range(iters):
            acc += pad[:, it]
        s = 128
        while s > 0:
            acc[:, :s] += acc[:, s:2 * s]
            s >>= 1
        part[j] = acc[:, 0]
    return part


def emulate_fold(slabs):
    """cs_fold_kernel's own order in fp32 over slabs (nsplit, n): thread group g of 16 adds the slabs g, g + 16, ... in order, the
    16 group sums are added in group order.  (n,) fp32."""
    slabs = np.ascontiguousarray(slabs, dtype=np.float32)
    acc = np.zeros((16, slabs.shape[1]), dtype=np.float32)
    for s in range(slabs.shape[0]):
        acc[s % 16] += slabs[s]
    v = np.zeros(slabs.shape[1], dtype=np.float32)
    for k in range(16):
        v += acc[k]
    return v


def emulate_fold_wide(slabs):
    """cs_fold_wide_kernel's own order in fp32: the slabs added in slab order."""
    v = np.zeros(slabs.shape[1], dtype=np.float32)
    for s in range(slabs.shape[0]):
        v += np.asarray(slabs[s], dtype=np.float32)
    return v


# ---- 5: the gather-GEMM's accumulator chain in the forward and the data gradient -------------------------------------------------------
# gg_kernel with nsplit = 1 adds an output's K products one after another into one fp32 accumulator (chunks of 16 k in order, two
# k per v_mfma_f32_32x32x2f32, in order).  torch's CPU convolution blocks its sums, so on the longest reductions -- K = 2304 for
# kind 0's last convolution, 1152 for the others named here -- the kernel's order is up to five times further from float64 than
# torch's, and three per-image rows of the fp32 mode came out between 1.00 and 1.32 of four torch distances on the MI355X when
# they were first held layer-locally ("The stacks at the batch sizes the update runs").  Those rows are bound by
# four times the distance of THIS order's emulation from float64 instead; the engine is not re-tiled for it.  (On the GPU's own
# buffers the emulation below gave the GPU's maps bit for bit.)
CHAIN_ROWS = {0: ("act.17", "g.7"), 1: ("act.14",), 2: ()}
CHAIN_DRAWS = 3         # (the emulation of g.7 takes a second per draw of four images)


def chain_conv_forward(x, w, b, stride, pad):
    """relu(conv(x, w) + b), every output's products added one at a time in k = (ci, ky, kx) order into one fp32 accumulator (one
    rounding per product: a fused multiply-add), the bias added in fp32 afterwards: gg_kernel<ConvFwdP>'s order.  fp32 tensor."""
    x, w = F.pad(cb.tt(x).double(), (pad,) * 4), cb.tt(w).double()
    ho = (x.shape[2] - 3) // stride + 1
    acc = torch.zeros(x.shape[0], w.shape[0], ho, ho, dtype=torch.float32)
    for ci in range(w.shape[1]):
        for ky in range(3):
            for kx in range(3):
                xs = x[:, ci:ci + 1, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (ho - 1) + 1:stride]
                acc = (acc.double() + xs * w[:, ci, ky, kx].view(1, -1, 1, 1)).float()
    return torch.relu(acc + cb.tt(b).float().view(1, -1, 1, 1))


def chain_data_grad(g, w, pad):
    """conv_transpose(g, w) of a stride-1 layer, ungated, every output's products added one at a time in k = (co, ky, kx) order
    into one fp32 accumulator: gg_kernel<ConvDgradP>'s order.  fp32 tensor of the layer input's shape."""
    g, w = F.pad(cb.tt(g).double(), (2 - pad,) * 4), cb.tt(w).double()
    h = g.shape[2] - 2
    acc = torch.zeros(g.shape[0], w.shape[1], h, h, dtype=torch.float32)
    for co in range(w.shape[0]):
        for ky in range(3):
            for kx in range(3):
                gs = g[:, co:co + 1, 2 - ky:2 - ky + h, 2 - kx:2 - kx + h]
                acc = (acc.double() + gs * w[co, :, ky, kx].view(1, -1, 1, 1)).float()
    return acc


def chain_row(kind, row, P, xs, maps):
    """One CHAIN_ROWS row in the kernel's own order, as a float64 numpy array: 'act.<l>' from the layer's input xs[l], 'g.<l>' from
    the g of the layer above and the map of layer l (maps: 'act.<l>' / 'g.<l>' fp32 tensors or arrays)."""
    geo = cb.geometry(kind)
    names = [n for n, *_ in geo]
    what, n = row.split(".")
    l = names.index(n)
    if what == "act":
        _n, _ci, _co, stride, pad, _pl = geo[l]
        return chain_conv_forward(xs[l], P[n + ".weight"], P[n + ".bias"], stride, pad).double().numpy()
    up, _ci, _co, stride, pad, _pl = geo[l + 1]
    assert stride == 1
    dx = chain_data_grad(cb.tt(maps["g." + up]).float(), P[up + ".weight"], pad)
    return cb.gate_below(dx, cb.tt(maps["act." + n]).float(), geo[l][5]).double().numpy()


_CHAIN = {}


def chain_bounds(kind, B=4):
    """{row: MARGIN * the largest distance of the row in the kernel's own order from float64 over CHAIN_DRAWS of
    convstack_bf16_cpu's draws at B images} for CHAIN_ROWS[kind]; memoised."""
    if (kind, B) not in _CHAIN:
        worst = {r: 0.0 for r in CHAIN_ROWS[kind]}
        for i in range(CHAIN_DRAWS if worst else 0):
            ops = cb.draw_operands(kind, B, cb.CASE_SEED + i, rounding=False)
            maps = {k: v for k, v in ops.items() if k.startswith(("act.", "g."))}
            xs = cb.layer_inputs(kind, ops["image"], maps)
            P = {k: v.numpy() for k, v in ops["P"].items()}
            d = {"image": ops["image"], "d_feat": np.zeros((B, cc.feat_width(kind)), dtype=np.float32)}
            for r in worst:
                what, n = r.split(".")
                ref = cb.layer_refs(kind, P, d, {k: v.numpy() for k, v in maps.items()}, what=(what,), layers=[n], rounding=False)[r]
                worst[r] = max(worst[r], cb.rel(chain_row(kind, r, P, xs, maps), ref))
        _CHAIN[(kind, B)] = {r: cb.MARGIN * v for r, v in worst.items()}
    return _CHAIN[(kind, B)]

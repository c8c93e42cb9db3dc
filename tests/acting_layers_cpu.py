"""Layer-by-layer CPU restatement of the two ACTING forwards (var_armnet_forward: csrc/armnet.hip, var_ithor_policy_forward:
csrc/ithor_policy.hip, over csrc/c3f.h, csrc/chain.h, csrc/actor_critic.h), the checker of tests/test_gpu_acting_layers.py: one
plain torch function per layer kind, each from the layer's own inputs to its output, in the dtype of what it is given (float64 =
the reference, float32 = torch's CPU kernels = the yardstick).

A model is a graph of such layers over named buffers (`graph("arm")`, `graph("ipol")`): the conv outputs a1..a8 / a1..a6, the
pooled maps p1..p3 / p1..p4, occf, and the vectors of the MLP under the lower-case names of the chain's schedule (cnn0, flat, m0,
m1, motor, s0, s1, sound, o0, occ, h0, gh, im0, x, f0, fusion, gi, hout, imr, all0, all1, c0, c1, a0, feats, value, head).  Which
of them a forward leaves behind depends on its route (`survivors`): up to 64 images the band kernels pool inside the launch
(no a2 / a4 / a6), up to 8 rows the chain keeps every vector, beyond that the per-layer path reuses its scratch rows.  A check
(`check_layers`) evaluates ONE surviving buffer from the nearest surviving buffers upstream of it -- the single layer where both
survive, the fused convolution + pool or a run of two or three Linear layers where an intermediate does not -- in float64 and
compares the device's buffer with it.  Nothing carries across checks.

The bound of a check (tests/trunk_cpu.py's convention): MARGIN times the distance of torch's fp32 CPU evaluation of the same
function on the same inputs from the float64 one, relative to the float64 array's largest magnitude.  Never the kernel's own
output.  Routing and selection (the pool of the device's own map, the mask) are exact in every precision: distance 0, bound 0.
For the layers of ORDER the yardstick is an fp32 emulation of the kernel's own accumulation order instead of torch's."""
import collections

import torch
import torch.nn.functional as F

from tests.ithor_layers_cpu import MARGIN, ratio, rel, scale  # noqa: F401  (one yardstick for every pin)

Node = collections.namedtuple("Node", "kind fn ins")
INPUTS = ("image", "occupancy", "image_feat", "robot_pose", "goal", "hxs", "masks")
OUTPUTS = ("value", "head", "hout")
MAPS = {"arm": ("a1", "a2", "p1", "a3", "a4", "p2", "a5", "a6", "p3", "a7", "a8"),
        "ipol": ("a1", "a2", "p1", "a3", "p2", "a4", "p3", "a5", "p4", "a6", "occf")}
BAND_MAX_B, CHAIN_ROWS = 64, 8                                    # csrc/image_stack.h: kBandMaxB, csrc/chain.h: kChainRows
# c3f::Cfg's band height TR of the band convolutions, by the buffer they write (csrc/armnet.hip, csrc/image_stack.h); conv 1: C1_TR
BAND_ROWS = {"arm": {"a1": 2, "p1": 4, "a3": 6, "p2": 6, "a5": 8, "p3": 4}, "ipol": {"a1": 2, "p1": 4, "p2": 6, "p3": 4, "p4": 4}}


# ---- layer kinds ---------------------------------------------------------------------------------------------------------------
def image_input(image, dtype):
    """The first three channels of a float image, or of a u8 image divided by 255, in `dtype`."""
    x = image[:, :3]
    return x.to(dtype) / 255 if image.dtype == torch.uint8 else x.to(dtype)


def conv3x3(x, w, b, stride=1, pad=1, pool=False, flat=False):
    """3x3 convolution + bias + ReLU, optionally with the 2x2 max pool the band kernels fuse, optionally flattened."""
    y = F.relu(F.conv2d(x, w, b, stride=stride, padding=pad))
    y = F.max_pool2d(y, 2, 2) if pool else y
    return y.flatten(1) if flat else y


def conv1(image, w, b):
    return conv3x3(image_input(image, w.dtype), w, b)


def pool2x2(x):
    return F.max_pool2d(x, 2, 2)


def occupancy_stage(occ, w0, b0, w1, b1):
    """occupancyCNNMLP's two convolutions (1 -> 64 -> 32, 3x3 stride 2 pad 1, ReLU each) of a (B, 1, 9, 9) map, flattened."""
    x = occ.to(w0.dtype) / 255 if occ.dtype == torch.uint8 else occ.to(w0.dtype)
    return conv3x3(conv3x3(x.reshape(-1, 1, 9, 9), w0, b0, 2, 1), w1, b1, 2, 1, flat=True)


def linear_input(form, xs):
    """The chain's input forms: 'plain' x, 'sum' (x0 + x1) (+ x2), 'cat' [x0 | x1], 'mask' h * mask (mask (B, 1))."""
    if form == "plain":
        return xs[0]
    if form == "sum":
        s = xs[0] + xs[1]
        return s + xs[2] if len(xs) > 2 else s
    if form == "cat":
        return torch.cat(xs, 1)
    assert form == "mask"
    return xs[0] * xs[1]


def linear(xs, w, b, relu=True, form="plain"):
    y = linear_input(form, xs) @ w.t() + b
    return F.relu(y) if relu else y


def mask_rows(h, masks):
    return h * masks


def gru_cell(gi, gh, h0):
    """torch.nn.GRU's cell (gate order r, z, n) from the two gate pre-activations (biases included) and the masked state."""
    H = h0.shape[1]
    r = torch.sigmoid(gi[:, :H] + gh[:, :H])
    z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    return (1 - z) * n + z * h0


# ---- the models as graphs ------------------------------------------------------------------------------------------------------
def graph(model):
    """{buffer: Node(kind, fn, ins)}: fn maps the buffers / inputs / parameters (state_dict keys) named by ins to the buffer."""
    G = {}

    def conv(out, x, key, stride=1, pad=1, flat=False):
        first = x == "image"
        G[out] = Node("conv", (lambda x, w, b: conv1(x, w, b)) if first else
                      (lambda x, w, b: conv3x3(x, w, b, stride, pad, flat=flat)), [x, f"base.imgCNN.{key}.weight", f"base.imgCNN.{key}.bias"])

    def pool(out, x):
        G[out] = Node("pool", pool2x2, [x])

    def lin(out, xs, key, relu=True, form="plain", names=None):
        w, b = names or (key + ".weight", key + ".bias")
        n = len(xs)
        G[out] = Node("linear", lambda *a: linear(a[:n], a[n], a[n + 1], relu, form), list(xs) + [w, b])

    conv("a1", "image", 0)
    conv("a2", "a1", 2)
    pool("p1", "a2")
    if model == "arm":
        conv("a3", "p1", 5), conv("a4", "a3", 7), pool("p2", "a4"), conv("a5", "p2", 10), conv("a6", "a5", 12), pool("p3", "a6")
        conv("a7", "p3", 15, 2, 0), conv("a8", "a7", 17, 1, 0, flat=True)
        last = "a8"
        lin("m0", ["image_feat", "robot_pose"], "base.motorMlp.0", form="cat")
        lin("m1", ["m0"], "base.motorMlp.2"), lin("motor", ["m1"], "base.motorMlp.4")
        lin("im0", ["flat", "motor"], "base.imgMotorMlp.0", form="sum")
        lin("head", ["feats"], "dist.fc_mean", relu=False)
    else:
        conv("a3", "p1", 5), pool("p2", "a3"), conv("a4", "p2", 8), pool("p3", "a4"), conv("a5", "p3", 11), pool("p4", "a5")
        conv("a6", "p4", 14, 2, 1, flat=True)
        last = "a6"
        occ = "base.occupancyCNNMLP."
        G["occf"] = Node("occupancy", occupancy_stage, ["occupancy", occ + "0.weight", occ + "0.bias", occ + "2.weight", occ + "2.bias"])
        lin("o0", ["occf"], occ + "5"), lin("occ", ["o0"], occ + "7")
        lin("m0", ["image_feat"], "base.motorMlp.0"), lin("motor", ["m0"], "base.motorMlp.2")
        lin("im0", ["flat", "motor", "occ"], "base.imgMotorMlp.0", form="sum")
        lin("head", ["feats"], "dist.linear", relu=False)
    lin("cnn0", [last], "base.cnnMlp.0"), lin("flat", ["cnn0"], "base.cnnMlp.2")
    lin("s0", ["goal"], "base.soundMlp.0"), lin("s1", ["s0"], "base.soundMlp.2"), lin("sound", ["s1"], "base.soundMlp.4")
    G["h0"] = Node("mask", mask_rows, ["hxs", "masks"])
    lin("gh", ["h0"], None, relu=False, names=("base.gru.weight_hh_l0", "base.gru.bias_hh_l0"))
    lin("x", ["im0"], "base.imgMotorMlp.2")
    lin("f0", ["sound", "flat"], "base.fusionMlp.0", form="sum"), lin("fusion", ["f0"], "base.fusionMlp.2")
    lin("gi", ["x"], None, relu=False, names=("base.gru.weight_ih_l0", "base.gru.bias_ih_l0"))
    G["hout"] = Node("gru", gru_cell, ["gi", "gh", "h0"])
    lin("imr", ["hout"], "base.imgMotorMlp2.0")
    lin("all0", ["fusion", "imr"], "base.mlp_all.0", form="sum"), lin("all1", ["all0"], "base.mlp_all.2")
    lin("c0", ["all1"], "base.critic.0"), lin("c1", ["c0"], "base.critic.2"), lin("value", ["c1"], "base.critic_linear", relu=False)
    lin("a0", ["all1"], "base.actor.0"), lin("feats", ["a0"], "base.actor.2")
    return G


def survivors(model, B, head=True):
    """The buffers a forward of B rows leaves behind, by the route it takes (graph order)."""
    G = graph(model)
    fused = ("a2", "a4", "a6") if model == "arm" else ("a2", "a3", "a4", "a5")
    maps = [k for k in MAPS[model] if not (B <= BAND_MAX_B and k in fused)]
    if B <= CHAIN_ROWS:
        rest = [k for k in G if k not in MAPS[model] and k != "h0"]
    else:      # the per-layer path: t0 = actor.0's, t1 = critic.2's, t2 = mlp_all.0's, t3 = mlp_all.2's output when it returns
        rest = ["flat", "motor", "sound", "fusion", "h0", "gi", "gh", "hout", "all0", "all1", "c1", "a0", "feats", "value", "head"]
        rest += ["occ"] if model == "ipol" else []
    return [k for k in G if (k in maps or k in rest) and (head or k != "head")]


def _cast(x, dtype):
    return x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x


def evaluate(G, out, env, P, dtype, override=None, used=None):
    """Buffer `out` in `dtype` from the nearest buffers of `env` upstream of it (never env[out] itself) and the parameters P.
    `override`: {buffer: fn} replacing a node's function (the order emulations, the injected faults); `used`: a list that
    receives (kind, buffer) of every node evaluated."""
    memo = {}

    def value(k):
        if k in P:
            return _cast(P[k], dtype)
        if k in env:
            return _cast(env[k], dtype)
        if k not in memo:
            memo[k] = run(k)
        return memo[k]

    def run(k):
        node = G[k]
        if used is not None:
            used.append((node.kind, k))
        fn = override[k] if override and k in override else node.fn
        return fn(*[value(i) for i in node.ins])

    return run(out)


def chain(model, P, inputs, override=None):
    """Every buffer of the model from its inputs, in the dtype of the parameters P."""
    dtype = next(iter(P.values())).dtype
    G, b = graph(model), dict(inputs)
    for k in G:
        b[k] = evaluate(G, k, b, P, dtype, override)
    return b


def layer_distance(G, out, env, P, order=None):
    """(float64 output, distance): the yardstick of one check -- largest |fp32 - float64| / largest |float64| of `out` evaluated
    from env; with `order` ({buffer: fp32 emulation of the kernel's accumulation order}) the emulation replaces torch's fp32."""
    ref = evaluate(G, out, env, P, torch.float64)
    f32 = evaluate(G, out, env, P, torch.float32, override=order)
    return ref, rel(f32, ref)


# ---- the kernels' own accumulation orders ------------------------------------------------------------------------------------
def seq_dot(A, B, step):
    """A (M, K) @ B (K, N) on ONE fp32 accumulator per output, `step` products per turn added in order, every operation rounded
    to fp32 (a matrix instruction's k: 4 for v_mfma_f32_16x16x4_f32, 2 for v_mfma_f32_32x32x2f32)."""
    A, B = A.float().t().contiguous(), B.float().contiguous()
    acc, p, q = (torch.zeros(A.shape[1], B.shape[1]) for _ in range(3))
    for k in range(0, A.shape[0], step):
        torch.mul(A[k, :, None], B[k], out=p)
        for j in range(k + 1, min(k + step, A.shape[0])):
            p += torch.mul(A[j, :, None], B[j], out=q)
        acc += p
    return acc


def band_order(cin):
    """k of csrc/c3f.h's product loop in filter order (ci * 9 + tap): 16-channel group, tap, four channels per instruction."""
    return [(16 * kg + 4 * j + c) * 9 + tap for kg in range(cin // 16) for tap in range(9) for j in range(4) for c in range(4)]


def conv3x3_seq(x, w, b, stride=1, pad=1, pool=False, flat=False, step=4, perm=None, ways=1):
    """conv3x3 with K on one accumulator (`ways` > 1: K split that many ways by 16-channel group, group g to way g % ways, the
    partial sums folded in order: c3f.h's c3s_kernel)."""
    cols = F.unfold(x.float(), 3, padding=pad, stride=stride).transpose(0, 1).flatten(1)          # (K, images * pixels)
    A = w.float().flatten(1)
    perm = list(range(A.shape[1])) if perm is None else perm
    y = None
    for way in range(ways):
        ks = [k for k in perm if (k // 144) % ways == way]
        part = seq_dot(A[:, ks], cols[ks], step)
        y = part if y is None else y + part
    y = F.relu(y + b.float()[:, None])
    ho = (x.shape[2] + 2 * pad - 3) // stride + 1
    y = y.reshape(w.shape[0], x.shape[0], ho, ho).transpose(0, 1)
    y = F.max_pool2d(y, 2, 2) if pool else y
    return y.flatten(1) if flat else y.contiguous()


def linear_seq(xs, w, b, relu=True, form="plain", step=2):
    y = seq_dot(w, linear_input(form, [t.float() for t in xs]).t(), step).t() + b.float()
    return F.relu(y) if relu else y


def linear_chain(xs, w, b, relu=True, form="plain"):
    """linear as csrc/chain.h's mlp_chain_kernel accumulates it: lane l of 64 takes k = l, l + 64, ... in order with one fused
    multiply-add each (fmaf: the exact product added in float64, then rounded to fp32), the 64 partial sums fold as a balanced
    tree (lanes l and l ^ 32, then ^ 16, 8, 4, 2, 1), the bias is added last."""
    x = linear_input(form, [t.float() for t in xs])
    K = x.shape[1]
    pad = (-K) % 64
    prod = F.pad(x.double()[:, None, :] * w.double()[None], (0, pad))                  # (rows, outputs, K): exact products
    acc = torch.zeros(prod.shape[0], prod.shape[1], 64)
    for j in range(0, K + pad, 64):
        acc = (acc.double() + prod[..., j:j + 64]).float()
    for h in (32, 16, 8, 4, 2, 1):
        acc = acc[..., :h] + acc[..., h:2 * h]
    y = acc[..., 0] + b.float()
    return F.relu(y) if relu else y


# CANDIDATES: the emulation of the kernel's own order for every product that runs over K >= 1024, and for the chain's value
# layer, by (model, node, route of that node), with the node's arguments.  ORDER: those measured on the MI355X beyond MARGIN x
# torch's fp32 distance with nothing but the accumulation order to blame (figures in DESIGN section 7):
#   arm a6 on the gather-GEMM route (B = 65): K = 1152 on ONE accumulator, 1.08 x the bound; 0.45 x the emulation's
#   arm value on the chain at B = 1: ONE number, 0.0151, the sum of 128 products of total magnitude 0.377 (condition 25); the
#     device is 7.5e-9 off, a third of an fp32 ulp of that magnitude, but 1.9 x the bound torch's single 1-ulp sample sets; the
#     emulation reproduces the device's bits
CANDIDATES = {
    ("arm", "a6", "gemm"): lambda x, w, b: conv3x3_seq(x, w, b, step=2),
    ("arm", "a7", "gemm"): lambda x, w, b: conv3x3_seq(x, w, b, 2, 0, step=2),
    ("arm", "a8", "gemm"): lambda x, w, b: conv3x3_seq(x, w, b, 1, 0, flat=True, step=2),
    ("arm", "a6", "band"): lambda x, w, b: conv3x3_seq(x, w, b, perm=band_order(128)),
    ("arm", "a7", "band"): lambda x, w, b: conv3x3_seq(x, w, b, 2, 0, ways=4),
    ("arm", "a8", "band"): lambda x, w, b: conv3x3_seq(x, w, b, 1, 0, flat=True, ways=4),
    ("ipol", "a6", "gemm"): lambda x, w, b: conv3x3_seq(x, w, b, 2, 1, flat=True, step=2),
    ("ipol", "a6", "band"): lambda x, w, b: conv3x3_seq(x, w, b, 2, 1, flat=True, ways=4),
    ("arm", "cnn0", "layer"): lambda x, w, b: linear_seq([x], w, b),
    ("ipol", "cnn0", "layer"): lambda x, w, b: linear_seq([x], w, b),
    ("ipol", "gh", "layer"): lambda x, w, b: linear_seq([x], w, b, relu=False),
    ("arm", "cnn0", "chain"): lambda x, w, b: linear_chain([x], w, b),
    ("ipol", "cnn0", "chain"): lambda x, w, b: linear_chain([x], w, b),
    ("ipol", "gh", "chain"): lambda x, w, b: linear_chain([x], w, b, relu=False),
    ("arm", "value", "chain"): lambda x, w, b: linear_chain([x], w, b, relu=False),
}
ORDER = {k: CANDIDATES[k] for k in (("arm", "a6", "gemm"), ("arm", "value", "chain"))}


def route_of(B, buffer, model):
    return ("band" if B <= BAND_MAX_B else "gemm") if buffer in MAPS[model] else ("chain" if B <= CHAIN_ROWS else "layer")


def order_for(model, B, table=None):
    """{node: emulation} for a forward of B rows, from ORDER (or from `table`)."""
    table = ORDER if table is None else table
    return {k: fn for (m, k, route), fn in table.items() if m == model and route == route_of(B, k, model)}


# ---- the checks ----------------------------------------------------------------------------------------------------------------
def check_layers(model, env, P, outputs, B=None, images=None, order=None, log=None):
    """Every buffer of `outputs` against float64 evaluated from the other buffers of env (the device's, with the inputs):
    {buffer: (what the check spans, error, distance, ratio)}.  `images`: the convolutions are compared on these images only (they
    are independent; pools and the MLP on every row).  `order`: {node: emulation}; a check that spans such a node takes the
    emulation's distance."""
    G, res = graph(model), {}
    for out in outputs:
        sub = images is not None and out in MAPS[model] and G[out].kind != "pool"
        e = {k: (v[images] if sub else v) for k, v in env.items() if k != out}
        used = []
        ref = evaluate(G, out, e, P, torch.float64, used=used)
        ov = {k: fn for k, fn in (order or {}).items() if k in [u for _kind, u in used]}
        dist = rel(evaluate(G, out, e, P, torch.float32, override=ov), ref)
        got = env[out][images] if sub else env[out]
        assert got.shape == ref.shape, (out, got.shape, ref.shape)
        err = rel(got, ref)
        span = "+".join(f"{kind}:{k}" for kind, k in reversed(used)) + (" (kernel order)" if ov else "")
        res[out] = (span, err, dist, ratio(err, dist))
        if log:
            log(f"{out:7s} {span:44s} err {err:.2e} dist {dist:.2e} ratio {res[out][3]:.3f}")
    return res


def end_to_end(model, P, inputs, got):
    """{output: (error, distance, ratio)} of value, head and hout against the float64 chain from the inputs; the distance is the
    fp32 chain's (torch's CPU kernels end to end)."""
    ref = chain(model, {k: v.double() for k, v in P.items()}, inputs)
    f32 = chain(model, {k: v.float() for k, v in P.items()}, inputs)
    out = {}
    for k in OUTPUTS:
        if k in got:
            err, dist = rel(got[k], ref[k]), rel(f32[k], ref[k])
            out[k] = (err, dist, ratio(err, dist))
    return out


def random_inputs(model, B, seed, u8=True, channels=3, masks=None):
    """Inputs of a forward by name (INPUTS): a random image (B, channels, 96, 96), u8 or float already divided by 255 (iTHOR's
    occupancy map in the same form), unit-length features, a hidden state of standard deviation 0.3, `masks` (default: every
    third row reset)."""
    g = torch.Generator().manual_seed(seed)
    H = 512 if model == "arm" else 1024
    unit = lambda n: F.normalize(torch.randn(B, n, generator=g), dim=1)      # noqa: E731
    img = torch.randint(0, 256, (B, channels, 96, 96), dtype=torch.uint8, generator=g)
    d = {"image": img if u8 else img.float() / 255, "image_feat": unit(3), "goal": unit(3),
         "hxs": torch.randn(B, H, generator=g) * 0.3,
         "masks": torch.tensor([[float(r % 3 != 1)] for r in range(B)]) if masks is None else torch.tensor(masks).float().view(B, 1)}
    if model == "arm":
        d["robot_pose"] = torch.randn(B, 2, generator=g)
    else:
        occ = (torch.rand(B, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255
        d["occupancy"] = occ if u8 else occ.float() / 255
    return d


# ---- faults (tests/test_acting_layers_host.py): each returns the faulty content of ONE buffer ---------------------------------
def _node_args(G, out, env, P):
    return [_cast(P[k] if k in P else env[k], torch.float32) for k in G[out].ins]


def faults(model, env, P, other):
    """[(fault, buffer, faulty fp32 content)] over a clean fp32 set of buffers `env` of the chain + band route (B <= 8; `other`:
    the same buffers of another call): what a wrong kernel would leave in that one buffer, everything upstream intact."""
    G = graph(model)
    tr = BAND_ROWS[model]
    out = []

    def last_column(k):
        y = env[k].clone()
        y[..., -1] = 0
        return y

    def fused(k, edit, w_edit=None):
        """the band convolution that writes k (with its pool when it fuses one), its un-pooled map edited"""
        conv = k if G[k].kind == "conv" else G[k].ins[0]
        x, w, b = _node_args(G, conv, env, P)
        y = G[conv].fn(x, w_edit(w) if w_edit else w, b)
        y = edit(y) if edit else y
        return pool2x2(y) if conv != k else y

    def band_row(k):
        def edit(y):
            y = y.clone()
            y[:, :, tr[k]] = 0
            return y
        return fused(k, edit)

    def drop_tap(k):
        def w_edit(w):      # the last tap of the first 16 input channels (one turn of the band kernels' product loop)
            w = w.clone()
            w[:, :16, 2, 2] = 0
            return w
        return fused(k, None, w_edit)

    convs = [k for k in survivors(model, CHAIN_ROWS) if k in MAPS[model] and k != "occf"]
    for k in convs:
        if env[k].dim() == 4:
            out.append(("last column zero", k, last_column(k)))
        out.append(("one tap dropped", k, drop_tap(k)))
    for k in tr:
        out.append(("first row of band 1 zero", k, band_row(k)))
    for k in tr:
        if G[k].kind == "pool":
            out.append(("pool over the wrong window", k, fused(k, lambda y: torch.roll(y, -1, -1))))
    for k in ("cnn0", "x", "value"):
        args = _node_args(G, k, env, P)
        out.append(("Linear fed the neighbouring row", k, G[k].fn(args[0].roll(1, 0), *args[1:])))
    for k in ("im0", "f0", "all0"):
        args = _node_args(G, k, env, P)
        n = len(args) - 2
        relu = lambda xs, w, b: F.relu(sum(xs[1:], xs[0]) @ w.t() + b)      # noqa: E731
        out.append(("sum missing its last addend", k, relu(args[:n - 1], args[n], args[n + 1])))
    w, b = (P[k].float() for k in G["gh"].ins[1:])
    out.append(("mask ignored", "gh", env["hxs"].float() @ w.t() + b))
    h0 = mask_rows(env["hxs"].float(), env["masks"].float())
    out.append(("mask ignored", "hout", gru_cell(env["gi"].float(), env["gh"].float(), env["hxs"].float())))
    H = h0.shape[1]
    swap = lambda g: torch.cat([g[:, H:2 * H], g[:, :H], g[:, 2 * H:]], 1)      # noqa: E731
    out.append(("r and z gates swapped", "hout", gru_cell(swap(env["gi"].float()), swap(env["gh"].float()), h0)))
    for k in ("p1", "cnn0", "gi", "hout", "feats"):
        y, o = env[k].clone(), other[k]
        d = (y - o).abs().flatten()
        big = (d > 1e-3 * scale(y)).nonzero()       # a stale value that differs by less than that is no fault to any fp32 check
        assert len(big), k
        y.view(-1)[big[0]] = o.reshape(-1)[big[0]]
        out.append(("one element left from the previous call", k, y))
    for k in ("a1", "p3", "gh", "c0", "head"):
        y = env[k].clone()
        y.view(-1)[y.numel() // 3] = float("nan")
        out.append(("a NaN", k, y))
    return out

"""Layer-by-layer CPU restatement of the frozen iTHOR encoder's reward step (csrc/ithor_reward.hip: var_ithor_reward_step over
csrc/c3f.h, csrc/image_stack.h, csrc/gg.h), the checker of tests/test_gpu_ithor_reward_layers.py: one plain torch function per
layer, each from the layer's own inputs to its output, in the dtype of what it is given (float64 = the reference, float32 =
torch's CPU kernels = the yardstick).  The yardstick and the layer functions it shares are tests/ithor_layers_cpu.py's.

Buffers carry var_debug_buffer's "irew_" names, cut to the batch that ran: a1 (B, 32, 96, 96), p1..p4 (the fused convolution +
pool outputs), a6 (B, 1152), hid (B, 128), s1 / s2 (clip, 64, h, w), s3 in the sequence layout (clip, 73, 448), gi (dir, clip,
73, 1536), gh (slab, dir, clip, 1536: above 16 clips only), h72 / h73 (clip, [forward 512 | reverse 512]: the two state slots
after a goal step, slot 0 and slot 1), hs1, hs2, graw, frozen; with the step's inputs (image, goal), its outputs (image_feat,
goal_feat, reward) and the parameter arena the pack read (arena).

`rows(route)` is the table of checks: each evaluates ONE surviving buffer from the nearest surviving buffers upstream of it.
Nothing carries across checks.  The GRU keeps two state slots only, so it is pinned twice: the LAST step alone (h73 from the
device's h72 and gi; above 16 clips also the sum of the device's gh slabs against h72 W_hh^T and h73 from those slabs through
the gate arithmetic), and the CHAIN (h72 from the device's gi by an unroll of 72 steps from a zero state).

The bound of a check: MARGIN times the distance of torch's fp32 CPU evaluation of the same function on the same inputs from the
float64 one, relative to the float64 array's largest magnitude.  Never the kernel's own output.  Copies (frozen) are exact:
bound 0.  For the rows of ORDER the yardstick is an fp32 emulation of the kernel's documented accumulation order instead."""
import collections

import torch
import torch.nn.functional as F

from tests import ithor_layers_cpu as lc
from tests.ithor_layers_cpu import GH, IMG, MARGIN, SND, T, ratio, rel, scale  # noqa: F401  (one yardstick for every pin)

FUSED_CLIPS, REC_SPLIT, BAND_MAX_B = 16, 4, 64            # csrc/ithor_reward.hip: kFusedClips, kRecSplit; image_stack.h: kBandMaxB
BAND_ROWS = {"a1": 2, "p1": 4, "p2": 6, "p3": 4, "p4": 4}          # band height of the kernel that writes the buffer (image_stack.h)
IMAGE_SIDE = ("a1", "p1", "p2", "p3", "p4", "a6", "hid", "image_feat")
SOUND_SIDE = ("s1", "s2", "s3", "gi", "gh", "h72", "h73", "hs1", "hs2", "graw")
OUTPUTS = ("image_feat", "goal_feat", "reward")
Row = collections.namedtuple("Row", "name out fn ins kind got", defaults=(None,))


def route_of(B):
    return "fused" if B <= FUSED_CLIPS else "split"


# ---- layers ----------------------------------------------------------------------------------------------------------------
def conv_pool(x, w, b):
    """A band kernel with the pool fused: 3x3 convolution + ReLU + 2x2 max pool."""
    return lc.pool_fwd(lc.conv_fwd(x, w, b, "i"))


def conv6(x, w, b):
    return lc.conv_fwd(x, w, b, "i6").flatten(1)


def linear_relu(x, w, b):
    return lc.linear_fwd(x, w, b, True)


def linear_plain(x, w, b):
    return lc.linear_fwd(x, w, b, False)


def head_out(hid, w, b):
    """Linear(128, 3) + F.normalize: what rw_tail_kernel's last workgroup makes of hid."""
    return lc.l2norm_fwd(lc.linear_fwd(hid, w, b, False))


def snd1(x, w, b):
    return lc.conv_fwd(x, w, b, "s1")


def snd2(x, w, b):
    return lc.conv_fwd(x, w, b, "s2")


def snd3(x, w, b):
    """The third sound convolution in the sequence layout, (clip, 73, 448)."""
    return lc.conv_fwd(x, w, b, "s3", seq=True).flatten(2)


def halves(h):
    """(clip, [forward 512 | reverse 512]) -> (dir, clip, 512)."""
    return torch.stack([h[:, :GH], h[:, GH:]])


def joined(h):
    return torch.cat([h[0], h[1]], 1)


def gru_last(h72, gi, w_hh, b_hh):
    """h_73 from h_72 and gi: direction 0 at t = 72, direction 1 at t = 0."""
    h, gs = halves(h72)[:, None], lc.by_step(gi)[:, T - 1:T]
    _, z, n, _ = lc._gates(h, gs, w_hh, b_hh)
    return joined(((1 - z) * n + z * h)[:, 0])


def gru_chain(gi, w_hh, b_hh, h0=None, forwards=False):
    """h_72 from gi by an unroll from a zero state (`h0`, `forwards`: the faults of tests/test_ithor_reward_layers_host.py -- a
    first step that reads a state, direction 1 walking time forwards)."""
    if h0 is None and not forwards:
        return joined(lc.gru_unroll(gi, w_hh, b_hh)[:, T - 1])
    gs = torch.stack([gi[0].transpose(0, 1), gi[1].transpose(0, 1)]) if forwards else lc.by_step(gi)
    h = torch.zeros(2, gi.shape[1], GH, dtype=gi.dtype) if h0 is None else halves(h0.to(gi.dtype))
    for s in range(T - 1):
        _, z, n, _ = lc._gates(h[:, None], gs[:, s:s + 1], w_hh, b_hh)
        h = ((1 - z) * n + z * h[:, None])[:, 0]
    return joined(h)


def rec_product(h72, w_hh):
    """h_72 W_hh^T without the bias, (dir, clip, 1536)."""
    return halves(h72) @ w_hh.transpose(1, 2)


def rec_slabs(h72, w_hh):
    """The product as REC_SPLIT split-K slabs (slab, dir, clip, 1536): the stand-in of the device's gh on the CPU."""
    h, q = halves(h72), GH // REC_SPLIT
    return torch.stack([h[..., s * q:(s + 1) * q] @ w_hh[..., s * q:(s + 1) * q].transpose(1, 2) for s in range(REC_SPLIT)])


def slab_sum(gh, nsplit=REC_SPLIT):
    """The slabs added in slab order (rw_gru_gate_kernel's loop)."""
    s = gh[0]
    for k in range(1, nsplit):
        s = s + gh[k]
    return s


def gru_gates(gh, gi, h72, b_hh, nsplit=REC_SPLIT, swap=False):
    """h_73 from the slabs of the recurrent product through the gate arithmetic (`nsplit`, `swap`: faults)."""
    g, gs, h = slab_sum(gh, nsplit) + b_hh[:, None, :], lc.by_step(gi)[:, T - 1], halves(h72)
    R, Z = (slice(GH, 2 * GH), slice(0, GH)) if swap else (slice(0, GH), slice(GH, 2 * GH))
    r = torch.sigmoid(gs[..., R] + g[..., R])
    z = torch.sigmoid(gs[..., Z] + g[..., Z])
    n = torch.tanh(gs[..., 2 * GH:] + r * g[..., 2 * GH:])
    return joined((1 - z) * n + z * h)


def reward_dot(image_feat, goal_feat):
    return (image_feat * goal_feat).sum(1)


def copy_of(x):
    return x


# ---- the table of checks -----------------------------------------------------------------------------------------------------
def params(P):
    """The state_dict with the GRU's four tensors stacked over the directions under rnn.w_ih / w_hh / b_ih / b_hh."""
    Q = dict(P)
    Q["rnn.w_ih"], Q["rnn.w_hh"], Q["rnn.b_ih"], Q["rnn.b_hh"] = lc.rnn_params(P)
    return Q


def arena_of(P):
    """The parameter arena: the state_dict's tensors in order (csrc/ithor_reward.hip: make_layout)."""
    return torch.cat([v.reshape(-1) for v in P.values()])


def rows(route, goal=True):
    """[Row(name, buffer checked, function, its inputs (buffers | parameters), kind, what of the buffer is compared)]; kind
    'conv': compared on chosen images, 'layer': on every row, 'exact': a copy.  `goal` False: an image-only step."""
    wb = lambda k: [k + ".weight", k + ".bias"]      # noqa: E731
    t = [Row("a1", "a1", lc.conv1_fwd, ["image"] + wb(IMG[0]), "conv")]
    for l, x in ((1, "a1"), (2, "p1"), (3, "p2"), (4, "p3")):
        t.append(Row(f"p{l}", f"p{l}", conv_pool, [x] + wb(IMG[l]), "conv"))
    t += [Row("a6", "a6", conv6, ["p4"] + wb(IMG[5]), "conv"),
          Row("hid", "hid", linear_relu, ["a6"] + wb("imgTriplet.0"), "layer"),
          Row("image_feat", "image_feat", head_out, ["hid"] + wb("imgTriplet.2"), "layer")]
    if goal:
        t += [Row("s1", "s1", snd1, ["goal"] + wb(SND[0]), "conv"), Row("s2", "s2", snd2, ["s1"] + wb(SND[1]), "conv"),
              Row("s3", "s3", snd3, ["s2"] + wb(SND[2]), "conv"),
              Row("gi", "gi", lc.gru_input, ["s3", "rnn.w_ih", "rnn.b_ih"], "layer"),
              Row("gru.chain", "h72", gru_chain, ["gi", "rnn.w_hh", "rnn.b_hh"], "layer")]
        if route == "split":
            t.append(Row("gru.gh", "gh", rec_product, ["h72", "rnn.w_hh"], "layer", slab_sum))
        t.append(Row("gru.last", "h73", gru_last, ["h72", "gi", "rnn.w_hh", "rnn.b_hh"], "layer"))
        if route == "split":
            t.append(Row("gru.gates", "h73", gru_gates, ["gh", "gi", "h72", "rnn.b_hh"], "layer"))
        t += [Row("hs1", "hs1", linear_relu, ["h73"] + wb("soundTriplet.0"), "layer"),
              Row("hs2", "hs2", linear_relu, ["hs1"] + wb("soundTriplet.2"), "layer"),
              Row("graw", "graw", linear_plain, ["hs2"] + wb("soundTriplet.4"), "layer"),
              Row("goal_feat", "goal_feat", lc.l2norm_fwd, ["graw"], "layer")]
    t += [Row("reward", "reward", reward_dot, ["image_feat", "goal_feat"], "layer"), Row("frozen", "frozen", copy_of, ["arena"], "exact")]
    return t


def steps(route):
    """The forward as a chain: (buffer, function, inputs) in order.  h73 comes from the slabs where the route has them."""
    skip = ("gru.gh", "gru.gates", "frozen") + (("gru.last",) if route == "split" else ())
    out = []
    for r in rows(route):
        if r.name == "gru.last" and route == "split":
            out += [("gh", rec_slabs, ["h72", "rnn.w_hh"]), ("h73", gru_gates, ["gh", "gi", "h72", "rnn.b_hh"])]
        if r.name not in skip:
            out.append((r.out, r.fn, r.ins))
    return out


def _cast(x, dtype):
    return x.to(dtype) if torch.is_tensor(x) and x.is_floating_point() else x


def chain(P, image, goal, route, start=None, changed=()):
    """Every buffer of a goal step from its inputs, in the dtype of the parameters P.  `start`, `changed`: the buffers of an
    earlier chain, of which those in `changed` were edited -- only what depends on them is evaluated again."""
    Q = params(P)
    dt = Q["rnn.w_hh"].dtype
    b = dict(start) if start else {"image": image, "goal": _cast(goal, dt), "arena": arena_of(P), "frozen": arena_of(P).clone()}
    dirty = set(changed)
    for out, fn, ins in steps(route):
        if start is not None and (out in dirty or not dirty & set(ins)):
            continue
        b[out] = fn(*[Q[k] if k in Q else b[k] for k in ins])
        dirty.add(out)
    return b


# ---- the kernels' own accumulation orders ------------------------------------------------------------------------------------
def snd2_order(x, w, b):
    """The second sound convolution as csrc/gg.h accumulates it (K = 64 x 11 x 5 = 3520 on ONE accumulator, two products per
    matrix instruction: ithor_layers_cpu.conv_fwd_seq), over the first and the last clip given; the distance is taken
    relative to the whole output's largest magnitude (a maximum over fewer outputs on the same scale: never the larger bound)."""
    return [0, -1], lc.conv_fwd_seq(x, w, b, "s2", [0, x.shape[0] - 1])


def order_distance(emu, x, ref):
    """Distance of an emulation from the float64 output `ref`: emu(*x) is the whole output, or (index, those entries of it)."""
    y = emu(*x)
    return rel(y[1], ref[y[0]], scale(ref)) if isinstance(y, tuple) else rel(y, ref)


# ORDER: the rows measured on the MI355X beyond MARGIN x torch's fp32 distance with nothing but the accumulation order to blame,
# by (row, route of the GRU | None for every route), with the emulation of the kernel's own order (figures in DESIGN section 7):
#   s2, the gather-GEMM's GS2 instantiation: 1.33 - 1.75 x the bound in all six cases, as the same kernel's row snd2.fwd of the
#   training path is (ithor_layers_cpu.ORDER: 1.3 - 1.9).  Every other row sits below its bound on torch's own yardstick
#   (worst: p3 0.82, graw 0.81 at B = 1, hs1 0.80); under the emulation s2 stands at 0.26 - 0.51.
ORDER = {("s2", None): snd2_order}


def order_for(route):
    return {name: fn for (name, r), fn in ORDER.items() if r is None or r == route}


# ---- the checks ----------------------------------------------------------------------------------------------------------------
def check_layers(env, P, route, goal=True, images=None, order=None, only=None, log=None):
    """Every row of rows(route, goal) on `env` (the device's buffers with the step's inputs and outputs):
    {row: (error, distance, ratio)}, error and distance relative to the float64 output's largest magnitude.  `images`: the
    convolutions are compared on these images / clips only (they are independent).  `order`: {row: emulation}.  `only`: the rows to run."""
    Q, res = params(P), {}
    for r in rows(route, goal):
        if only is not None and r.name not in only:
            continue
        sub = images is not None and r.kind == "conv"
        ins = [Q[k] if k in Q else env[k] for k in r.ins]
        x = [ins[0][images] if sub else ins[0]] + ins[1:]
        ref = r.fn(*[_cast(v, torch.float64) for v in x])
        emu = (order or {}).get(r.name)
        dist = order_distance(emu, x, ref) if emu else rel(r.fn(*[_cast(v, torch.float32) for v in x]), ref)
        g = r.got(env[r.out]) if r.got else env[r.out]
        g = g[images] if sub else g
        assert g.shape == ref.shape, (r.name, g.shape, ref.shape)
        err = rel(g, ref)
        res[r.name] = (err, dist, ratio(err, dist))
        if log:
            e, d, q = res[r.name]
            log(f"{r.name:10s} {'(kernel order) ' if (order or {}).get(r.name) else ''}err {e:.2e} dist {d:.2e} ratio {q:.3f}")
    return res


# ---- faults (tests/test_ithor_reward_layers_host.py) ---------------------------------------------------------------------------
Fault = collections.namedtuple("Fault", "what buffer value fails P", defaults=(None,))


def zero_head(P, head):
    """The parameters with the last Linear of a head ('imgTriplet.2' | 'soundTriplet.4') set to zero: its raw output is 0."""
    return dict(P, **{head + ".weight": torch.zeros_like(P[head + ".weight"]), head + ".bias": torch.zeros_like(P[head + ".bias"])})


def faults(env, P, route, other, plan):
    """[Fault(what, buffer, its faulty fp32 content, rows that must fail, parameters if not P)] over a clean fp32 set of buffers
    `env` (`other`: the same of another call; `plan` > B: the planned batch): what a wrong kernel would leave in that ONE buffer,
    everything upstream intact.  The rows that must fail are those that check the buffer."""
    Q = params(P)
    w_hh, b_hh = Q["rnn.w_hh"], Q["rnn.b_hh"]
    B = env["image"].shape[0]
    out = []
    table = {r.name: r for r in rows(route)}
    own = lambda k: tuple(r.name for r in rows(route) if r.out == k)      # noqa: E731

    def add(what, k, y, fails=None, P_=None):
        out.append(Fault(what, k, y, own(k) if fails is None else fails, P_))

    def args(name):
        return [Q[k] if k in Q else env[k] for k in table[name].ins]

    def fused(k, edit=None, w_edit=None):
        x, w, b = args(k)
        y = lc.conv_fwd(x, w_edit(w) if w_edit else w, b, "i")
        return lc.pool_fwd(edit(y) if edit else y)

    def zeroed(y, *idx):
        y = y.clone()
        y[idx] = 0
        return y

    def no_tap(w):      # the last tap of the first 16 input channels (one turn of the band kernels' product loop)
        w = w.clone()
        w[:, :16, -1, -1] = 0
        return w

    # convolutions and pools
    add("last column zero", "a1", zeroed(env["a1"], Ellipsis, -1))
    add("last column zero", "p1", fused("p1", lambda y: zeroed(y, Ellipsis, -1)))
    add("last column zero", "s1", zeroed(env["s1"], Ellipsis, -1))
    add("last column zero", "s3", zeroed(env["s3"].view(B, T, 64, 7), Ellipsis, -1).view(B, T, -1))
    for k in ("a1", "p1", "p2", "p3", "p4"):
        row = (slice(None), slice(None), BAND_ROWS[k])
        add("first row of band 1 zero", k, zeroed(env[k], *row) if k == "a1" else fused(k, lambda y, row=row: zeroed(y, *row)))
    for k in ("p2", "p4"):
        add("one tap dropped", k, fused(k, None, no_tap))
    x, w, b = args("a6")
    add("one tap dropped", "a6", conv6(x, no_tap(w), b))
    x, w, b = args("s2")
    add("one tap dropped", "s2", snd2(x, no_tap(w), b))
    for k in ("p1", "p3"):
        add("pool over the wrong window", k, fused(k, lambda y: torch.roll(y, -1, -1)))
    # the tail
    x, w, b = args("hid")
    add("ReLU missing", "hid", x @ w.t() + b)
    add("last 16-byte piece of the weight row taken twice", "hid", F.relu(x @ w.t() + b + x[:, -4:] @ w[:, -4:].t()))
    add("Linear fed the neighbouring row", "hid", linear_relu(x.roll(1, 0), w, b))
    zi, zs = zero_head(P, "imgTriplet.2"), zero_head(P, "soundTriplet.4")
    add("normalisation floor missing (raw output 0)", "image_feat", torch.full_like(env["image_feat"], float("nan")), None, zi)
    add("normalisation floor missing (raw output 0)", "goal_feat", torch.full_like(env["goal_feat"], float("nan")), None, zs)
    add("rows rolled by one", "goal_feat", env["goal_feat"].roll(1, 0))
    add("formed from the previous goal", "reward", reward_dot(env["image_feat"], other["goal_feat"]))
    # the GRU
    gi, h72 = env["gi"], env["h72"]
    flat = F.pad(gi.reshape(-1), (0, (plan - B) * T * 3 * GH))
    at_plan = torch.stack([gi[0], flat[plan * T * 3 * GH:][:B * T * 3 * GH].view(B, T, -1)])
    last = (lambda *a, **kw: gru_gates(env["gh"], *a, **kw)) if route == "split" else None
    h73 = lambda gi=gi, h=h72, bh=b_hh, **kw: (last(gi, h, bh, **kw) if last else gru_last(h, gi, w_hh, bh))      # noqa: E731
    add("direction 1 read at the plan's stride, not B's", "h73", h73(gi=at_plan))
    wrong_clip = h72.clone()
    wrong_clip[B - 1] = h72[0]
    add("the last clip served from another clip's column", "h73", gru_last(wrong_clip, gi, w_hh, b_hh))
    swap = lambda g: torch.cat([g[..., GH:2 * GH], g[..., :GH], g[..., 2 * GH:]], -1)      # noqa: E731
    add("r and z gates swapped", "h73", gru_gates(env["gh"], gi, h72, b_hh, swap=True) if last else
        gru_last(h72, swap(gi), torch.cat([w_hh[:, GH:2 * GH], w_hh[:, :GH], w_hh[:, 2 * GH:]], 1), swap(b_hh)))
    add("b_hh missing", "h73", h73(bh=torch.zeros_like(b_hh)))
    add("direction 1 walking time forwards", "h72", gru_chain(gi, w_hh, b_hh, forwards=True))
    add("direction 1 walking time forwards", "h73", gru_last(h72, torch.stack([gi[0], gi[1].flip(1)]), w_hh, b_hh))
    # (a FINITE state at step 0 is forgotten long before step 72 -- tests/test_ithor_reward_layers_host.py measures 6e-14 -- so
    # the state that shows an ignored `first` flag is the one the GPU test plants: NaN)
    add("step 0 reading a NaN state", "h72", gru_chain(gi, w_hh, b_hh, h0=torch.full_like(h72, float("nan"))))
    add("a clip's column clamped to its neighbour", "h72", gru_chain(torch.cat([gi[:, :B - 1], gi[:, B - 2:B - 1]], 1), w_hh, b_hh))
    if route == "split":
        add("the gate kernel adds three of the four slabs", "h73", gru_gates(env["gh"], gi, h72, b_hh, nsplit=REC_SPLIT - 1))
        # (h73 follows the slabs it is given, so gru.gates holds; the slabs' own row and the last step from h72 do not)
        add("slab 3 left unwritten by the product", "gh", zeroed(env["gh"], REC_SPLIT - 1), ("gru.gh", "gru.last"))
    # anywhere
    for k in ("p2", "a6", "gi", "h73", "hs2", "graw", "frozen") + (("gh",) if route == "split" else ()):
        y, o = env[k].clone(), other[k] if k != "frozen" else env[k] + 1e-2
        d = (y - o).abs().flatten()
        big = (d > 1e-3 * scale(y)).nonzero()       # a stale value that differs by less than that is no fault to any fp32 check
        assert len(big), k
        y.view(-1)[big[0]] = o.reshape(-1)[big[0]]
        add("one element left from the previous call", k, y, ("gru.gh", "gru.last") if k == "gh" else None)
    for k in ("a1", "p4", "hid", "s2", "gi", "h72", "hs1", "image_feat", "reward"):
        y = env[k].clone()
        y.view(-1)[y.numel() // 3] = float("nan")
        add("a NaN", k, y)
    return out

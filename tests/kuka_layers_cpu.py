"""Layer-by-layer CPU restatement of the Kuka VARPretextNet's training step (oracle.torch_oracle.KukaNetCPU; on the device
img_head2 / img_mid3 / img_chain / img_wgrad345 / img_tail2, snd_*, heads_*), the checker of tests/test_gpu_kuka_layers.py: one
plain torch function per layer kind and direction, each from the layer's own inputs to its outputs, in the dtype of what it is
given (float64 = the reference, float32 = torch's CPU kernels = the yardstick).  The bound, rel, ratio, layer_eval, seq_dot and
the Linear / l2-norm helpers are tests/ithor_layers_cpu.py's own.

Buffers carry var_debug_buffer's names, cut to the batch that ran: act1..act5 (B, C, h, h), sact1..sact4 (clips, 32, T, 1) with
clips = [positive | negative] (a call without one half holds the other alone), hid_i (B, 128), hid_s (clips, 128), the heads'
rows with the suffix _i (images) and _s (clips): raw (emb_raw), emb, gemb, graw (the first three of graw's four floats per row),
ghid; parameter gradients as "G." + the state_dict name.

Which gradient a g-buffer holds, READ IN THE KERNELS (not guessed): every gact* / gsact* buffer holds the gradient AFTER its own
layer's ReLU mask, i.e. wrt the layer's pre-activation --
  gact5 / gsact4   heads_bwd_gemm_kernel / heads_bwd_fused_kernel: gx = ghid W0 "masked by x > 0", x = act5 / sact4;
  gact4, gact3, gact2   img_chain.hip: "gx = (W^T (*) gy) . (x > 0)", the mask applied before the store the weight gradients read;
  gsact3..gsact1   snd_dgrad_kernel: "g4 -> g3 -> g2 -> g1 (each masked by its activation > 0)";
  ghid             heads_bwd_rows*_kernel: (graw W1) zeroed where hid is not positive;
  gact1            never exists in HBM: img_tail2 keeps its masked band in LDS (its block is the scratch of the act1 untile that
                   var_debug_buffer("act1") launches), so conv 1's weight and bias gradients are ONE composed row from gact2,
                   conv 2's filter, act1's mask and the image.
So a weight / bias gradient row takes its g-buffer as it is, and a data-gradient row masks its output with the activation the
output belongs to.  Masks always come from the buffers handed in (the device's own activations)."""
import torch
import torch.nn.functional as F

from tests.ithor_layers_cpu import (FLIP_RATE, MARGIN, _tuple, conv_bgrad, l2norm_bwd, l2norm_fwd, layer_distance,  # noqa: F401
                                    layer_eval, linear_bwd, linear_fwd, linear_fwd_seq, ratio, rel, relu_mask, scale, seq_dot)

ICH = (3, 32, 32, 64, 64, 64)
SND_T = (100, 48, 23, 11, 5)
IMG = tuple(f"imgBranch.{2 * l}" for l in range(5))
SND = tuple(f"soundCNN.{2 * l}" for l in range(4))
IGEO = ((2, 2), (1, 1))                                            # stride, padding
SGEO = ((2, 1), (0, 0))
MARGIN_TRIPLET, EPS_TRIPLET = 1.0, 1e-6


def sides(h):
    """Image side lengths: the input, then the outputs of conv 1..5."""
    hs = [h]
    for _ in range(5):
        hs.append((hs[-1] - 1) // 2 + 1)
    return hs


# ---- convolutions ------------------------------------------------------------------------------------------------------------
def image_input(image, like):
    """The first three channels of a float image, or of a u8 image divided by 255 IN FP32 (dataset.py:67-68: the quotient the
    network is fed is an fp32 number), then widened to like's dtype."""
    x = image[:, :3]
    return (x.float() / 255).to(like.dtype) if image.dtype == torch.uint8 else x.to(like.dtype)


def conv_fwd(x, w, b, geo):
    return F.relu(F.conv2d(x, w, b, stride=geo[0], padding=geo[1]))


def conv1_fwd(image, w, b):
    return conv_fwd(image_input(image, w), w, b, IGEO)


def conv_dgrad(gy, w, geo, x):
    """Gradient wrt the pre-activation of the layer that produced x (post-ReLU), from gy (wrt this layer's pre-activation)."""
    dx = torch.nn.grad.conv2d_input(tuple(x.shape), w, gy, stride=geo[0], padding=geo[1])
    return dx * (x > 0)


def conv_wgrad(x, gy, geo, w_shape):
    return torch.nn.grad.conv2d_weight(x, tuple(w_shape), gy, stride=geo[0], padding=geo[1])


def conv1_grads(gact2, w2, act1, image, w1_shape):
    """(dW, db) of conv 1: conv 2's data gradient masked by act1 (never stored by the device), then conv 1's own products."""
    g1 = conv_dgrad(gact2, w2, IGEO, act1)
    return conv_wgrad(image_input(image, gact2), g1, IGEO, w1_shape), conv_bgrad(g1)


# ---- heads -------------------------------------------------------------------------------------------------------------------
def head_bwd2(hid, w1, graw):
    """dW1, db1 and the masked hidden gradient from the gradient wrt the un-normalised embedding."""
    return linear_bwd(hid, w1, graw, hid)


def head_bwd0(x, w0, ghid):
    """dW0, db0 and dX masked by x (= gact5 / gsact4 once reshaped)."""
    return linear_bwd(x, w0, ghid, x)


def triplet(a, p, n, margin, inv_count):
    """torch.nn.TripletMarginLoss(margin, p=2, eps=1e-6) times B * inv_count, and its gradients wrt the three (normalised)
    embeddings; a hinge argument of exactly zero is inactive (include/var_hip.h)."""
    dp, dn = a - p + EPS_TRIPLET, a - n + EPS_TRIPLET
    dap, dan = dp.norm(dim=1, keepdim=True), dn.norm(dim=1, keepdim=True)
    l = dap - dan + margin
    s = (l > 0).to(a.dtype) * inv_count
    up, un = dp / dap, dn / dan
    return (l.clamp_min(0).sum() * inv_count).reshape(1), s * (up - un), -s * up, s * un


def fused_heads(raw_i, raw_s, hid_i, hid_s, act5, sact4, wi0, wi1, ws0, ws1, margin, inv_count):
    """The fused training step's head: from the un-normalised embeddings (B images, 2B clips = [positive | negative]) the loss
    value, the eight head gradient tensors and gact5 / gsact4, every product in one go."""
    B = raw_i.shape[0]
    emb_i, emb_s = l2norm_fwd(raw_i), l2norm_fwd(raw_s)
    loss, ga, gp, gn = triplet(emb_i, emb_s[:B], emb_s[B:], margin, inv_count)
    dwi1, dbi1, ghid_i = head_bwd2(hid_i, wi1, l2norm_bwd(raw_i, ga))
    dws1, dbs1, ghid_s = head_bwd2(hid_s, ws1, l2norm_bwd(raw_s, torch.cat([gp, gn])))
    dwi0, dbi0, gx_i = head_bwd0(act5.flatten(1), wi0, ghid_i)
    dws0, dbs0, gx_s = head_bwd0(sact4.flatten(1), ws0, ghid_s)
    return loss, dwi0, dbi0, dwi1, dbi1, dws0, dbs0, dws1, dbs1, gx_i.view_as(act5), gx_s.view_as(sact4)


FUSED_OUT = ("loss", "G.imgTriplet.0.weight", "G.imgTriplet.0.bias", "G.imgTriplet.2.weight", "G.imgTriplet.2.bias",
             "G.soundTriplet.0.weight", "G.soundTriplet.0.bias", "G.soundTriplet.2.weight", "G.soundTriplet.2.bias", "gact5", "gsact4")


# ---- the whole model through the layer functions ------------------------------------------------------------------------------
def chain(P, image, snd, gemb_i=None, gemb_s=None, gates=None, forward=None, fault=None, fused=None):
    """Forward (and, with cotangents on the embeddings or with fused = (margin, inv_count), backward) of the model as a chain of
    the layer functions, in the dtype of the parameters P (state_dict names).  image (B, >= 3, h, h) u8 | float or None, snd
    (clips, 1, 100, 40) = [positive | negative] or None.  Returns every buffer under its debug name.  `gates` (activations by
    name, e.g. the device's): the backward takes every ReLU mask from them instead of from its own forward -- the gradient of
    the network with its gates held fixed.  `forward`: the buffers of an earlier forward of the same call, not run again.
    `fault` {buffer: fn}: the buffer is replaced by fn(buffer, the buffers so far) as soon as it exists and everything after it is computed from the
    replaced one -- what a kernel with that fault leaves behind (tests/test_kuka_layers_host.py)."""
    b = dict(forward or {})
    dt = P[SND[0] + ".weight"].dtype
    act = lambda k: gates[k].to(dt) if gates is not None and k in gates else b[k]      # noqa: E731

    def put(k, v):
        b[k] = fault[k](v, b) if fault and k in fault else v

    if image is not None and "act1" not in b:
        b["image"] = image
        put("act1", conv1_fwd(image, P[IMG[0] + ".weight"], P[IMG[0] + ".bias"]))
        for l in range(2, 6):
            put(f"act{l}", conv_fwd(b[f"act{l - 1}"], P[IMG[l - 1] + ".weight"], P[IMG[l - 1] + ".bias"], IGEO))
        put("hid_i", linear_fwd(b["act5"].flatten(1), P["imgTriplet.0.weight"], P["imgTriplet.0.bias"], True))
        put("raw_i", linear_fwd(b["hid_i"], P["imgTriplet.2.weight"], P["imgTriplet.2.bias"], False))
        put("emb_i", l2norm_fwd(b["raw_i"]))
    if snd is not None and "sact1" not in b:
        b["snd"] = snd.to(dt)
        for l in range(1, 5):
            x = b["snd"] if l == 1 else b[f"sact{l - 1}"]
            put(f"sact{l}", conv_fwd(x, P[SND[l - 1] + ".weight"], P[SND[l - 1] + ".bias"], SGEO))
        put("hid_s", linear_fwd(b["sact4"].flatten(1), P["soundTriplet.0.weight"], P["soundTriplet.0.bias"], True))
        put("raw_s", linear_fwd(b["hid_s"], P["soundTriplet.2.weight"], P["soundTriplet.2.bias"], False))
        put("emb_s", l2norm_fwd(b["raw_s"]))
    if fused is not None:
        B = b["emb_i"].shape[0]
        loss, gemb_i, gp, gn = triplet(b["emb_i"], b["emb_s"][:B], b["emb_s"][B:], *fused)
        put("loss", loss)
        gemb_s = torch.cat([gp, gn])
    if image is not None and gemb_i is not None:
        b["gemb_i"] = gemb_i.to(dt)
        put("graw_i", l2norm_bwd(b["raw_i"], b["gemb_i"]))
        dw, db, g = linear_bwd(b["hid_i"], P["imgTriplet.2.weight"], b["graw_i"], act("hid_i"))
        put("G.imgTriplet.2.weight", dw), put("G.imgTriplet.2.bias", db), put("ghid_i", g)
        dw, db, g = linear_bwd(b["act5"].flatten(1), P["imgTriplet.0.weight"], b["ghid_i"], act("act5").flatten(1))
        put("G.imgTriplet.0.weight", dw), put("G.imgTriplet.0.bias", db), put("gact5", g.view_as(b["act5"]))
        for l in range(5, 1, -1):
            w = P[IMG[l - 1] + ".weight"]
            put(f"G.{IMG[l - 1]}.weight", conv_wgrad(b[f"act{l - 1}"], b[f"gact{l}"], IGEO, w.shape))
            put(f"G.{IMG[l - 1]}.bias", conv_bgrad(b[f"gact{l}"]))
            if l > 2:
                put(f"gact{l - 1}", conv_dgrad(b[f"gact{l}"], w, IGEO, act(f"act{l - 1}")))
        dw, db = conv1_grads(b["gact2"], P[IMG[1] + ".weight"], act("act1"), b["image"], P[IMG[0] + ".weight"].shape)
        put(f"G.{IMG[0]}.weight", dw), put(f"G.{IMG[0]}.bias", db)
    if snd is not None and gemb_s is not None:
        b["gemb_s"] = gemb_s.to(dt)
        put("graw_s", l2norm_bwd(b["raw_s"], b["gemb_s"]))
        dw, db, g = linear_bwd(b["hid_s"], P["soundTriplet.2.weight"], b["graw_s"], act("hid_s"))
        put("G.soundTriplet.2.weight", dw), put("G.soundTriplet.2.bias", db), put("ghid_s", g)
        dw, db, g = linear_bwd(b["sact4"].flatten(1), P["soundTriplet.0.weight"], b["ghid_s"], act("sact4").flatten(1))
        put("G.soundTriplet.0.weight", dw), put("G.soundTriplet.0.bias", db), put("gsact4", g.view_as(b["sact4"]))
        for l in range(4, 0, -1):
            w = P[SND[l - 1] + ".weight"]
            x = b["snd"] if l == 1 else b[f"sact{l - 1}"]
            put(f"G.{SND[l - 1]}.weight", conv_wgrad(x, b[f"gsact{l}"], SGEO, w.shape))
            put(f"G.{SND[l - 1]}.bias", conv_bgrad(b[f"gsact{l}"]))
            if l > 1:
                put(f"gsact{l - 1}", conv_dgrad(b[f"gsact{l}"], w, SGEO, act(f"sact{l - 1}")))
    return b


# ---- the single-layer checks over a dict of buffers ----------------------------------------------------------------------------
def layer_table(b, P, fused=None):
    """[(name, kind, fn, inputs, outputs)]: every layer whose inputs and outputs are all in `b` (a chain's buffers, or the
    device's), as the function that maps these inputs (taken from `b`, with the parameters P) to the float64 / fp32 outputs and
    the buffers or arena slices ("G." names) that must hold them.  `kind` groups layers of one kernel kind and direction.  The
    g-buffers hold gradients wrt PRE-activations (after their own layer's mask: the module's docstring says where that was
    read), so weight and bias rows take them as they are and a data-gradient row masks with the activation of its output.
    fused = (margin, inv_count): the fused training step's one row "fused.heads" (loss, eight tensors, gact5, gsact4 from the
    device's own raw embeddings, hidden rows and features) takes the place of the heads' backward rows, whose intermediates
    (gemb, graw, ghid) that step does not keep."""
    rows = []

    def add(name, kind, fn, inputs, outputs):
        keys = [k for k in inputs + outputs if isinstance(k, str)]
        if all(k in b or k in P for k in keys):
            get = lambda k: (b[k] if k in b else P[k]) if isinstance(k, str) else k      # noqa: E731
            rows.append((name, kind, fn, [get(k) for k in inputs], [get(k) for k in outputs]))

    def gW(name):
        return "G." + name

    add("conv1.fwd", "img conv fwd", conv1_fwd, ["image", IMG[0] + ".weight", IMG[0] + ".bias"], ["act1"])
    for l in range(2, 6):
        w, c = IMG[l - 1] + ".weight", IMG[l - 1] + ".bias"
        add(f"conv{l}.fwd", "img conv fwd", lambda x, w, c: conv_fwd(x, w, c, IGEO), [f"act{l - 1}", w, c], [f"act{l}"])
        add(f"conv{l}.wgrad", "img conv wgrad", lambda x, g, s=tuple(P[w].shape): conv_wgrad(x, g, IGEO, s),
            [f"act{l - 1}", f"gact{l}"], [gW(w)])
        add(f"conv{l}.bgrad", "img conv bgrad", conv_bgrad, [f"gact{l}"], [gW(c)])
        if l > 2:
            add(f"conv{l}.dgrad", "img conv dgrad", lambda g, w, x: conv_dgrad(g, w, IGEO, x), [f"gact{l}", w, f"act{l - 1}"],
                [f"gact{l - 1}"])
    add("conv1.grads", "img conv2 dgrad + conv1 wgrad, bgrad", lambda g, w2, a, im, s=tuple(P[IMG[0] + ".weight"].shape): conv1_grads(g, w2, a, im, s),
        ["gact2", IMG[1] + ".weight", "act1", "image"], [gW(IMG[0] + ".weight"), gW(IMG[0] + ".bias")])
    for l in range(1, 5):
        x = "snd" if l == 1 else f"sact{l - 1}"
        w, c = SND[l - 1] + ".weight", SND[l - 1] + ".bias"
        add(f"snd{l}.fwd", "snd conv fwd", lambda x, w, c: conv_fwd(x, w, c, SGEO), [x, w, c], [f"sact{l}"])
        add(f"snd{l}.wgrad", "snd conv wgrad", lambda x, g, s=tuple(P[w].shape): conv_wgrad(x, g, SGEO, s), [x, f"gsact{l}"], [gW(w)])
        add(f"snd{l}.bgrad", "snd conv bgrad", conv_bgrad, [f"gsact{l}"], [gW(c)])
        if l > 1:
            add(f"snd{l}.dgrad", "snd conv dgrad", lambda g, w, x: conv_dgrad(g, w, SGEO, x), [f"gsact{l}", w, x], [f"gsact{l - 1}"])
    for side, feat, gfeat, lin in (("i", "act5", "gact5", "imgTriplet"), ("s", "sact4", "gsact4", "soundTriplet")):
        pre = "img" if side == "i" else "snd"
        add(f"{pre}_head0.fwd", "linear fwd", lambda x, w, c: linear_fwd(x.flatten(1), w, c, True),
            [feat, lin + ".0.weight", lin + ".0.bias"], ["hid_" + side])
        add(f"{pre}_head2.fwd", "linear fwd", lambda x, w, c: linear_fwd(x, w, c, False),
            ["hid_" + side, lin + ".2.weight", lin + ".2.bias"], ["raw_" + side])
        add(f"{pre}_l2norm.fwd", "l2norm fwd", l2norm_fwd, ["raw_" + side], ["emb_" + side])
        if fused is None:
            add(f"{pre}_l2norm.bwd", "l2norm bwd", l2norm_bwd, ["raw_" + side, "gemb_" + side], ["graw_" + side])
            add(f"{pre}_head2.bwd", "linear bwd", lambda h, w, g: head_bwd2(h, w, g)[::2], ["hid_" + side, lin + ".2.weight", "graw_" + side],
                [gW(lin + ".2.weight"), "ghid_" + side])
            add(f"{pre}_head2.bgrad", "linear bgrad", lambda g: g.sum(0), ["graw_" + side], [gW(lin + ".2.bias")])
            add(f"{pre}_head0.bwd", "linear bwd", lambda x, w, g: (lambda t: (t[0], t[2].view_as(x)))(head_bwd0(x.flatten(1), w, g)),
                [feat, lin + ".0.weight", "ghid_" + side], [gW(lin + ".0.weight"), gfeat])
            add(f"{pre}_head0.bgrad", "linear bgrad", lambda g: g.sum(0), ["ghid_" + side], [gW(lin + ".0.bias")])
    if fused is not None:
        add("fused.heads", "fused heads bwd", lambda *a, m=fused: fused_heads(*a, *m),
            ["raw_i", "raw_s", "hid_i", "hid_s", "act5", "sact4", "imgTriplet.0.weight", "imgTriplet.2.weight",
             "soundTriplet.0.weight", "soundTriplet.2.weight"], list(FUSED_OUT))
    return rows


def bias_sum_seq(g):
    """Column sums of g (rows, C) as heads_bwd_gemm_kernel's tile_gemm forms a bias gradient: wave w of four walks the steps
    s = w, w + 4, ... of two rows each, lane half h adding row 2 s + h to its own fp32 accumulator; a wave's sum is half 0 + half 1,
    the total (wave 0 + wave 1) + (wave 2 + wave 3)."""
    g = g.float()
    R, waves = g.shape[0], []
    for w in range(4):
        halves = []
        for h in (0, 1):
            acc = torch.zeros(g.shape[1])
            for st in range(w, (R + 1) // 2, 4):
                if 2 * st + h < R:
                    acc = acc + g[2 * st + h]
            halves.append(acc)
        waves.append(halves[0] + halves[1])
    return (waves[0] + waves[1]) + (waves[2] + waves[3])


# Rows whose yardstick is an fp32 emulation of the kernel's own accumulation order instead of torch's fp32 kernels: name ->
# (inputs -> (index, emulation of output[index])).  A row enters only after it MISSED MARGIN x torch's distance on the MI355X by a
# rounding-sized amount that the order explains (DESIGN section 2 records each); none is entered in advance.
#   snd_head2.bgrad   case D (4 clips): db1 = (g0 + g1) + (g2 + g3) on the device, ((g0 + g1) + g2) + g3 in torch, whose three
#                     additions happened to round to within 4.4e-9 of float64 -- a tenth of what ONE rounding to fp32 may cost
#                     (6.0e-8); the device's 7.0e-8 is a single unit in the last place of the largest entry.
ORDER = {
    "snd_head2.bgrad": lambda g: (slice(None), bias_sum_seq(g)),
}


def check_layers(b, P, only=None, log=None, fused=None):
    """Run every check of layer_table(b, P) (those whose name `only` accepts): {name: (kind, [(error, distance, ratio)] per
    output)}, error and distance relative to the float64 output's largest magnitude."""
    out = {}
    for name, kind, fn, inputs, outputs in layer_table(b, P, fused):
        if only is not None and not only(name):
            continue
        ref, dist = layer_eval(fn, inputs, ORDER.get(name))
        assert len(ref) == len(outputs) == len(dist), name
        res = []
        for got, r, d in zip(outputs, ref, dist):
            assert got.shape == r.shape, (name, got.shape, r.shape)
            e = rel(got, r)
            res.append((e, d, ratio(e, d)))
        out[name] = (kind, res)
        if log:
            log(f"{name:16s} {kind:14s} " + "  ".join(f"err {e:.2e} dist {d:.2e} ratio {q:.2f}" for e, d, q in res))
    return out


# ---- end to end ----------------------------------------------------------------------------------------------------------------
GATED = ("act1", "act2", "act3", "act4", "act5", "hid_i", "sact1", "sact2", "sact3", "sact4", "hid_s")
FORWARD = GATED + ("image", "raw_i", "emb_i", "snd", "raw_s", "emb_s")


def end_to_end(P, image, snd, gemb_i, gemb_s, dev):
    """The device's embeddings and gradient arena (`dev`: its buffers, "G.*" included) against the float64 chain (= float64
    autograd of the oracle, tests/test_kuka_layers_host.py).  A ReLU network's gradient jumps where a pre-activation crosses zero
    between two precisions, so (ithor_layers_cpu.end_to_end's rule) the float64 backward is taken AT THE DEVICE'S gates, and
    every unit whose gate differs from the float64 forward's must be a near-tie: the float64 / device value that passed the
    gate within MARGIN forward distances of zero.  The yardstick is torch's fp32 chain against float64, its backward at the
    float64 gates (so that a flip of its own cannot inflate it).  Returns ({name: (error, distance)} for emb_i, emb_s, arena
    and every "G." tensor, [(buffer, count, largest value, allowance)] of the flips, number of gated units)."""
    P64 = {k: v.double() for k, v in P.items()}
    snd64 = None if snd is None else snd.double()
    ref = chain(P64, image, snd64, gemb_i, gemb_s)
    f32 = chain(P, image, snd, gemb_i, gemb_s, gates={k: ref[k] for k in GATED if k in ref})
    at_dev = chain(P64, image, snd64, gemb_i, gemb_s, gates={k: dev[k] for k in GATED if k in dev},
                   forward={k: v for k, v in ref.items() if k in FORWARD})
    names = [k for k in P if "G." + k in ref]
    arena = lambda b: torch.cat([b["G." + k].reshape(-1).double() for k in names])      # noqa: E731
    out = {k: (rel(dev[k], ref[k]), rel(f32[k], ref[k])) for k in ("emb_i", "emb_s") if k in ref}
    out["arena"] = (rel(arena(dev), arena(at_dev)), rel(arena(f32), arena(ref)))
    out.update({"G." + k: (rel(dev["G." + k], at_dev["G." + k]), rel(f32["G." + k], ref["G." + k])) for k in names})
    flips, units = [], 0
    for k in GATED:
        if k not in ref:
            continue
        tol, d = MARGIN * rel(f32[k], ref[k]) * scale(ref[k]), dev[k].double()
        units += d.numel()
        m = (d > 0) != (ref[k] > 0)
        if m.any():
            flips.append((k, int(m.sum()), float(torch.maximum(d, ref[k])[m].max()), tol))
    return out, flips, units


# ---- the cases of tests/test_gpu_kuka_layers.py (shared with the host test, which shows that these very inputs keep the fp32
# stand-in within the flip cap) ----------------------------------------------------------------------------------------------------
CONV2 = ("conv1.fwd", "conv2.fwd", "conv1.grads", "conv2.wgrad", "conv2.bgrad")
CASES = {
    "A": dict(h=84, B=1, u8=False, ch=3, neg=True, seed=11),
    "B": dict(h=84, B=3, u8=True, ch=4, neg=False, seed=12),
    "C": dict(h=96, B=5, u8=False, ch=3, neg=True, seed=13),
    "D": dict(h=96, B=2, u8=False, ch=3, neg=True, seed=14, plan=5),
    "E": dict(h=84, B=37, u8=True, ch=3, neg=True, seed=15),
    "F": dict(h=96, B=37, u8=False, ch=3, neg=True, seed=16,
              only=("conv2.wgrad", "conv3.wgrad", "conv4.wgrad", "conv3.dgrad", "conv4.dgrad", "conv5.dgrad")),
    "G": dict(h=84, B=65, u8=True, ch=3, neg=True, seed=17, only=("snd", "conv2.wgrad")),
    "H": dict(h=84, B=129, u8=True, ch=3, neg=True, seed=18,
              only=("conv3.wgrad", "conv4.wgrad", "conv3.dgrad", "conv4.dgrad", "conv5.dgrad")),
    "I84": dict(h=84, B=257, u8=True, ch=3, neg=True, seed=19, only=CONV2),
    "I96": dict(h=96, B=257, u8=False, ch=3, neg=True, seed=20, only=CONV2),
}


def seeded_params(seed, h=84):
    """The parameters of a VARPretextNet built under torch.manual_seed(seed) (the reference constructor's draws), on the CPU."""
    import types

    import var_amd
    torch.manual_seed(seed)
    m = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 100, 40), representationDim=3))
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


def make_inputs(spec):
    """(image, clips = [positive | negative] or the positive ones alone, cotangent of the image rows, of the clip rows)."""
    import numpy as np
    h, B = spec["h"], spec["B"]
    rng = np.random.default_rng(100 + spec["seed"])
    img = rng.integers(0, 256, size=(B, spec["ch"], h, h), dtype=np.uint8)
    snd = (rng.standard_normal((2 * B, 1, 100, 40)) * 4.0).astype(np.float32)
    image = torch.from_numpy(img) if spec["u8"] else (torch.from_numpy(img) / 255.).float()
    cot = torch.from_numpy(rng.standard_normal((3 * B, 3)).astype(np.float32))
    n = 2 * B if spec["neg"] else B
    return image, torch.from_numpy(snd[:n]), cot[:B], cot[B:B + n]
